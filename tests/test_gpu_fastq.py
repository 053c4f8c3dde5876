"""FASTQ input through the C-ABI (needs a GPU).

A small device stage rewrites FASTQ records in place into text the FASTA parsers read as the same
reads (fk_fastq.inc); everything behind it is the FASTA path.  Expected results always come from
the CPU oracle on the equivalent FASTA, built here in Python from the same records: header '@' ->
'>', the sequence line kept, the '+' and quality lines dropped, and with min_quality = q every base
whose ord(quality) - offset < q replaced by 'N'.  The product's own FASTA path is never the
expectation.

Base input: the 3000 reads of fk.synth_fasta(3000, 100, 200_000), qualities from a seeded RNG over
Phred 2..40, some quality lines forced to begin with '@', '+' and '>': ~650 KB, ~20 map tiles.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import fastkmer_amd as fk
import oracle
from test_gpu_parity import assert_same_as_oracle
from test_gpu_comm import assert_union_matches_oracle

pytestmark = pytest.mark.gpu

CONFIGS = [(28, 10, 64), (55, 12, 64)]


# ---- records <-> FASTQ / equivalent FASTA

def qualities(rng, n, i, offset=33):
    q = bytearray((rng.integers(2, 41, n) + offset).astype(np.uint8).tobytes())
    if n and i % 4 == 0:
        q[0] = b"@+>"[i // 4 % 3]  # quality lines that begin like a header, a '+' line, a FASTA header
    return bytes(q)


def make_records(reads, seed, offset=33):
    rng = np.random.default_rng(seed)
    return [(b"r%010d" % i, s, b"r%010d" % i if i % 9 == 0 else b"", qualities(rng, len(s), i, offset))
            for i, s in enumerate(reads)]


def fastq_bytes(records, eol=b"\n"):
    return b"".join(b"@" + n + eol + s + eol + b"+" + p + eol + q + eol for n, s, p, q in records)


def mask(seq, qual, min_q, offset):
    if not min_q or not seq:
        return seq
    s = np.frombuffer(seq, dtype=np.uint8).copy()
    low = np.frombuffer(qual, dtype=np.uint8).astype(np.int64) - offset < min_q
    s[low] = ord("N")
    return s.tobytes()


def fasta_bytes(records, min_q=0, offset=33, eol=b"\n"):
    return b"".join(b">" + n + eol + mask(s, q, min_q, offset) + eol for n, s, p, q in records)


def masked_count(records, min_q, offset):
    return int(sum(int((np.frombuffer(q, dtype=np.uint8).astype(np.int64) - offset < min_q).sum())
                   for _, _, _, q in records))


def synth_reads():
    fasta = fk.synth_fasta(3000, 100, 200_000, seed=0xF0)
    lines = fasta.split(b"\n")
    return [lines[i] for i in range(1, len(lines), 2)]


def recut(reads, seed, lo=30, hi=250):
    """The same bases as reads of lo..hi bp, so that cuts fall in every line of a record."""
    rng = np.random.default_rng(seed)
    allb = b"".join(reads)
    out, pos = [], 0
    while pos < len(allb):
        n = int(rng.integers(lo, hi + 1))
        out.append(allb[pos:pos + n])
        pos += n
    return out


class Case:
    def __init__(self, records):
        self.records = records
        self.fastq = fastq_bytes(records)
        self._refs = {}

    def ref(self, k, m, B, min_q=0, offset=33):
        key = (k, m, B, min_q, offset)
        if key not in self._refs:
            self._refs[key] = oracle.OracleResult(fasta_bytes(self.records, min_q, offset), k, m, B)
        return self._refs[key]


@pytest.fixture(scope="module")
def base():
    c = Case(make_records(synth_reads(), 1))
    assert 600_000 < len(c.fastq) < 700_000
    return c


@pytest.fixture(scope="module")
def variable():
    c = Case(make_records(recut(synth_reads(), 2), 3))
    assert min(len(r[1]) for r in c.records[:-1]) >= 30 and max(len(r[1]) for r in c.records) > 240
    return c


def count(data, k, m, B=64, use_ht=False, **fmt):
    kc = fk.KmerCounter(k, m, 3, B, use_ht, input_format="fastq", **fmt)
    kc.ingest(data)
    kc.finish()
    return kc


def check(kc, ref, nrecords, ordered=True):
    st = kc.stats()
    assert st["kmers"] == ref.total_kmers and st["distinct"] == ref.distinct
    info = kc.fastq_info()
    assert info["records"] == nrecords and info["first_malformed"] is None
    assert_same_as_oracle(kc, ref, ordered=ordered)


# ---- 1. parity

@pytest.mark.parametrize("use_ht", [False, True])
@pytest.mark.parametrize("k,m,B", CONFIGS)
def test_parity_every_bin(base, k, m, B, use_ht):
    with count(base.fastq, k, m, B, use_ht) as kc:
        check(kc, base.ref(k, m, B), 3000, ordered=not use_ht)
        st = kc.stats()
        assert st["fasta_bytes"] == len(base.fastq) and st["fused_map"] == 1 and st["fused_fallback"] == 0
        # sequence bytes and one separator per header line the parser sees: three a record
        assert st["positions"] == 3000 * 100 + 3 * 3000
        assert kc.fastq_info()["masked_bases"] == 0
        assert kc.input_format() == ("fastq", 0, 33)


# ---- 2. quality masking

@pytest.mark.parametrize("offset", [33, 64])
def test_quality_masking(offset):
    records = make_records(synth_reads(), 5, offset)
    data = fastq_bytes(records)
    k, m, B = CONFIGS[0]
    ref = oracle.OracleResult(fasta_bytes(records, 20, offset), k, m, B)
    want = masked_count(records, 20, offset)
    assert 0.3 * 300_000 < want < 0.7 * 300_000  # about half of the bases
    with count(data, k, m, B, min_quality=20, quality_offset=offset) as kc:
        check(kc, ref, 3000)
        assert kc.fastq_info()["masked_bases"] == want


def test_quality_masking_of_every_base(base):
    k, m, B = CONFIGS[0]
    with count(base.fastq, k, m, B, min_quality=41) as kc:
        st = kc.stats()
        assert st["kmers"] == 0 and st["distinct"] == 0 and not kc.bin_sizes().any()
        info = kc.fastq_info()
        assert info == {"records": 3000, "masked_bases": 300_000, "first_malformed": None}


# ---- 3. streaming

@pytest.fixture
def small_segments(monkeypatch):
    monkeypatch.setenv("FASTKMER_INGEST_SEG", "65536")
    monkeypatch.setenv("FASTKMER_PIECE_BYTES", "65536")


@pytest.mark.parametrize("k,m,B", CONFIGS)
def test_streamed_pinned_segments(small_segments, variable, k, m, B):
    import torch
    data = variable.fastq
    host = torch.empty(len(data), dtype=torch.uint8).pin_memory()
    host.numpy()[:] = np.frombuffer(data, dtype=np.uint8)
    with fk.KmerCounter(k, m, 3, B, input_format="fastq") as kc:
        for _ in range(2):  # twice: the second job reuses the stage's buffers
            kc.ingest_ptr(host.data_ptr(), len(data))
            kc.finish()
            check(kc, variable.ref(k, m, B), len(variable.records))
            st = kc.stats()
            assert st["pieces_counted"] > 0 and st["fused_map"] == 1
    assert host.numpy().tobytes() == data  # the caller's bytes are read only


@pytest.mark.parametrize("chunk", [1009, 70_001])
def test_streamed_chunks(variable, chunk):
    k, m, B = CONFIGS[0]
    data = variable.fastq
    with fk.KmerCounter(k, m, 3, B, input_format="fastq") as kc:
        for i in range(0, len(data), chunk):
            kc.ingest_chunk(data[i:i + chunk], i + chunk >= len(data))
        kc.finish()
        check(kc, variable.ref(k, m, B), len(variable.records))
        streamed = [kc.get_bin(b) for b in range(B)]
    with count(data, k, m, B) as one:  # the one-shot result, bin by bin
        for b in range(B):
            keys, cnt = one.get_bin(b)
            assert np.array_equal(keys, streamed[b][0]) and np.array_equal(cnt, streamed[b][1]), b


def test_streamed_chunks_without_a_last_flag(variable):
    # no fk_ingest(..., last = 1): fk_finish ends the input (the rest behind the frontier is
    # normalised there, each byte once)
    k, m, B = CONFIGS[0]
    data = variable.fastq
    with fk.KmerCounter(k, m, 3, B, input_format="fastq") as kc:
        for i in range(0, len(data), 50_021):
            kc.ingest_chunk(data[i:i + 50_021], False)
        kc.finish()
        check(kc, variable.ref(k, m, B), len(variable.records))


# ---- 4. fallback paths

def test_two_kernel_map(monkeypatch, variable):
    monkeypatch.setenv("FASTKMER_FUSED", "0")
    k, m, B = CONFIGS[0]
    with count(variable.fastq, k, m, B) as kc:
        assert kc.stats()["fused_map"] == 0
        check(kc, variable.ref(k, m, B), len(variable.records))
    with fk.KmerCounter(k, m, 3, B, input_format="fastq") as kc:
        for i in range(0, len(variable.fastq), 70_001):
            kc.ingest_chunk(variable.fastq[i:i + 70_001], i + 70_001 >= len(variable.fastq))
        kc.finish()
        check(kc, variable.ref(k, m, B), len(variable.records))


def test_long_record_falls_back(base):
    rng = np.random.default_rng(11)
    long_read = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 10_000)].tobytes()
    # placed so that a map tile (32 512 bytes) starts ~5000 bytes into the long sequence line: further
    # than the fused map's 4096-byte read-back for the line holding a tile's start
    tile_start, size, at = 10 * 32_512, 0, 0
    while size < tile_start - 5500:
        size += len(fastq_bytes(base.records[at:at + 1]))
        at += 1
    assert tile_start - 5500 <= size < tile_start - 5000
    records = list(base.records[:at]) + [(b"long", long_read, b"", qualities(rng, 10_000, 1))] + \
        list(base.records[at:])
    k, m, B = CONFIGS[0]
    ref = oracle.OracleResult(fasta_bytes(records), k, m, B)
    with count(fastq_bytes(records), k, m, B) as kc:
        st = kc.stats()
        assert st["fused_fallback"] & 1 and st["fused_map"] == 0
        check(kc, ref, 3001)


def test_record_longer_than_the_frontier_scan(base):
    # the host looks at most 16 MiB back for the frontier: a 17 MiB read between short ones, streamed in
    # 4 MiB chunks, holds the frontier at its start until the record after it is seen
    rng = np.random.default_rng(13)
    n = 17 << 20
    # mostly N (no k-mers: the oracle stays quick), 50 000 real bases in the middle
    mid = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 50_000)].tobytes()
    long_read = b"N" * (n // 2) + mid + b"N" * (n - n // 2 - len(mid))
    qual = (rng.integers(2, 41, n, dtype=np.uint8) + 33).astype(np.uint8).tobytes()
    records = list(base.records[:300]) + [(b"long", long_read, b"", qual)] + list(base.records[300:600])
    data = fastq_bytes(records)
    k, m, B = CONFIGS[0]
    ref = oracle.OracleResult(fasta_bytes(records), k, m, B)
    with fk.KmerCounter(k, m, 3, B, input_format="fastq") as kc:
        for i in range(0, len(data), 4 << 20):
            kc.ingest_chunk(data[i:i + (4 << 20)], i + (4 << 20) >= len(data))
        kc.finish()
        assert kc.stats()["fused_fallback"] & 1
        check(kc, ref, 601)


# ---- 5. a borrowed device input

@pytest.mark.parametrize("shift", [0, 1])
def test_ingest_device_leaves_the_buffer_alone(base, shift):
    import torch
    k, m, B = CONFIGS[0]
    data = base.fastq
    dev = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    dev[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    before = dev.cpu().numpy().tobytes()
    with fk.KmerCounter(k, m, 3, B, input_format="fastq", min_quality=20) as kc:
        kc.ingest_device(dev.data_ptr() + shift, len(data))
        kc.finish()
        check(kc, base.ref(k, m, B, 20, 33), 3000)
        assert kc.fastq_info()["masked_bases"] == masked_count(base.records, 20, 33)
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == before


# ---- 6. edge inputs

def small_records():
    reads = synth_reads()[:40]
    return make_records(reads, 21)


def test_empty_input():
    with count(b"", 28, 10) as kc:
        st = kc.stats()
        assert st["kmers"] == 0 and st["distinct"] == 0 and st["fasta_bytes"] == 0
        assert kc.fastq_info() == {"records": 0, "masked_bases": 0, "first_malformed": None}


EDGES = {
    "no final newline": lambda r: (fastq_bytes(r)[:-1], fasta_bytes(r), len(r)),
    "crlf": lambda r: (fastq_bytes(r, b"\r\n"), fasta_bytes(r, eol=b"\r\n"), len(r)),
    "crlf, no final newline": lambda r: (fastq_bytes(r, b"\r\n")[:-2], fasta_bytes(r, eol=b"\r\n"), len(r)),
    "trailing blank lines": lambda r: (fastq_bytes(r) + b"\n\n\n\n\n", fasta_bytes(r), len(r)),
    "trailing blank crlf lines": lambda r: (fastq_bytes(r, b"\r\n") + b"\r\n\r\n", fasta_bytes(r, eol=b"\r\n"), len(r)),
    "zero-length read": lambda r: (fastq_bytes(r[:20] + [(b"empty", b"", b"", b"")] + r[20:]),
                                   fasta_bytes(r[:20] + [(b"empty", b"", b"", b"")] + r[20:]), len(r) + 1),
    "zero-length read last": lambda r: (fastq_bytes(r + [(b"empty", b"", b"", b"")]),
                                        fasta_bytes(r + [(b"empty", b"", b"", b"")]), len(r) + 1),
    "zero-length read last, blank lines": lambda r: (fastq_bytes(r + [(b"empty", b"", b"", b"")]) + b"\n\n",
                                                     fasta_bytes(r + [(b"empty", b"", b"", b"")]), len(r) + 1),
    "+name lines": lambda r: (fastq_bytes([(n, s, n, q) for n, s, p, q in r]), fasta_bytes(r), len(r)),
    "lowercase and N": lambda r: (fastq_bytes([(n, s[:30] + b"acgtNNRYn" + s[39:], p, q) for n, s, p, q in r]),
                                  fasta_bytes([(n, s[:30] + b"acgtNNRYn" + s[39:], p, q) for n, s, p, q in r]), len(r)),
    "one record shorter than k": lambda r: (fastq_bytes([(b"s", b"ACGTACGTAC", b"", b"IIIIIIIIII")]),
                                            fasta_bytes([(b"s", b"ACGTACGTAC", b"", b"IIIIIIIIII")]), 1),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_inputs(name):
    data, fasta, nrec = EDGES[name](small_records())
    k, m, B = CONFIGS[0]
    ref = oracle.OracleResult(fasta, k, m, B)
    with count(data, k, m, B) as kc:
        check(kc, ref, nrec)
    with fk.KmerCounter(k, m, 3, B, input_format="fastq") as kc:  # and in chunks, cuts in every line
        for i in range(0, len(data), 97):
            kc.ingest_chunk(data[i:i + 97], i + 97 >= len(data))
        kc.finish()
        check(kc, ref, nrec)


# ---- 7. malformed input

def _malformed_cases():
    r = small_records()
    r = [(n, s, n, q.replace(b"+", b"I").replace(b"@", b"I")) for n, s, p, q in r]  # "+name" lines
    rec = lambda i: fastq_bytes(r[i:i + 1])
    head, tail = fastq_bytes(r[:7]), fastq_bytes(r[8:])
    n7, s7, p7, q7 = r[7]
    whole, last = fastq_bytes(r[:39]), rec(39)
    l1 = len(b"@" + r[39][0] + b"\n")
    l2 = l1 + len(r[39][1]) + 1
    l3 = l2 + len(b"+" + r[39][2] + b"\n")
    return {
        "missing + line": (head + b"@" + n7 + b"\n" + s7 + b"\n" + q7 + b"\n" + tail, 7),
        "header without @": (head + n7 + b"\n" + s7 + b"\n+\n" + q7 + b"\n" + tail, 7),
        "quality one byte short": (head + b"@" + n7 + b"\n" + s7 + b"\n+\n" + q7[:-1] + b"\n" + tail, 7),
        "truncated in line 1": (whole + last[:l1 - 4], 39),
        "truncated in line 2": (whole + last[:l1 + 50], 39),
        "truncated in line 3": (whole + last[:l2 + 3], 39),
        "truncated in line 4": (whole + last[:l3 + 50], 39),
    }


@pytest.mark.parametrize("name", sorted(_malformed_cases()))
@pytest.mark.parametrize("chunk", [0, 211])
def test_malformed_input(name, chunk):
    data, bad = _malformed_cases()[name]
    k, m, B = CONFIGS[0]
    with fk.KmerCounter(k, m, 3, B, input_format="fastq") as kc:
        if chunk:
            for i in range(0, len(data), chunk):
                kc.ingest_chunk(data[i:i + chunk], i + chunk >= len(data))
        else:
            kc.ingest(data)
        with pytest.raises(fk.FastKmerError) as e:
            kc.finish()
        assert e.value.code == -1 and "FASTQ record %d " % bad in str(e.value), str(e.value)
        assert kc.fastq_info()["first_malformed"] == bad
        # the context takes a new job: FASTA, format set back
        kc.set_input_format("fasta")
        fasta = fasta_bytes(small_records())
        kc.ingest(fasta)
        kc.finish()
        assert_same_as_oracle(kc, oracle.OracleResult(fasta, k, m, B))
        # and a well-formed FASTQ job after that
        kc.set_input_format("fastq")
        kc.ingest(fastq_bytes(small_records()))
        kc.finish()
        check(kc, oracle.OracleResult(fasta, k, m, B), 40)


# ---- 8. two in-process ranks

def _two_ranks(feed, k, m, B):
    ctxs = [fk.KmerCounter(k, m, 3, B, n_ranks=2, rank=r, input_format="fastq") for r in range(2)]
    fk.comm_init_local(ctxs)
    errs = [None, None]

    def work(r):
        try:
            feed(ctxs[r], r)
            ctxs[r].finish()
        except Exception as e:  # noqa: BLE001 -- reported below
            errs[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a rank did not finish"
    for e in errs:
        if e is not None:
            raise e
    return ctxs


def test_two_ranks_split_and_file_range(tmp_path, variable):
    k, m, B = CONFIGS[0]
    path = tmp_path / "reads.fq"
    path.write_bytes(variable.fastq)
    ref = variable.ref(k, m, B)
    splits = [fk.split_bytes_fastq(str(path), 2, r) for r in range(2)]
    assert b"".join(splits) == variable.fastq and all(splits)
    ctxs = _two_ranks(lambda kc, r: kc.ingest(splits[r]), k, m, B)
    assert_union_matches_oracle(ctxs, ref)
    assert sum(c.fastq_info()["records"] for c in ctxs) == len(variable.records)
    for c in ctxs:
        c.close()
    ctxs = _two_ranks(lambda kc, r: kc.ingest_file_range(str(path)), k, m, B)
    assert_union_matches_oracle(ctxs, ref)
    assert sum(c.stats()["fasta_bytes"] for c in ctxs) == len(variable.fastq)
    for c in ctxs:
        c.close()


# ---- 9. state rules, and the calls that follow the format

def test_state_rules(base):
    k, m, B = CONFIGS[0]
    with fk.KmerCounter(k, m, 3, B) as kc:
        assert kc.input_format() == ("fasta", 0, 33)
        with pytest.raises(fk.FastKmerError) as e:
            kc.fastq_info()
        assert e.value.code == -2
        for bad in (0, 32, 65):
            with pytest.raises(fk.FastKmerError) as e:
                kc.set_input_format("fastq", 0, bad)
            assert e.value.code == -1
        with pytest.raises(fk.FastKmerError) as e:
            kc.set_input_format("fastq", -1, 33)
        assert e.value.code == -1
        assert fk.lib().fk_set_input_format(kc._h, 2, 0, 33) == -1
        assert kc.input_format() == ("fasta", 0, 33)
        kc.set_input_format("fastq", 5, 64)
        assert kc.input_format() == ("fastq", 5, 64)
        kc.set_input_format("fastq")
        kc.ingest_chunk(base.fastq[:100_000], False)
        with pytest.raises(fk.FastKmerError) as e:
            kc.set_input_format("fasta")
        assert e.value.code == -2
        kc.ingest_chunk(base.fastq[100_000:], True)
        kc.finish()
        check(kc, base.ref(k, m, B), 3000)
        kc.set_input_format("fasta")  # between jobs again
        kc.set_input_format("fastq")
        with pytest.raises(fk.FastKmerError) as e:  # documented: the file sampler reads FASTA only
            kc.balance_bins_file("/nonexistent.fq")
        assert e.value.code == -1
    with pytest.raises(fk.FastKmerError) as e:
        fk.KmerCounter(k, m, 3, B, sequence_type=1, input_format="fastq")
    assert e.value.code == -1
    with pytest.raises(ValueError):
        fk.KmerCounter(k, m, 3, B, input_format="bam")


def test_signature_counts_and_balance_follow_the_format(base):
    k, m, B = CONFIGS[0]
    want = oracle.bin_signatures(fasta_bytes(base.records), k, m)
    with fk.KmerCounter(k, m, 3, B, input_format="fastq") as kc:
        kc.ingest(base.fastq)
        got = kc.signature_counts().cpu().numpy()
        assert np.array_equal(got, want)
        kc.finish()  # the input stays ingested, normalised once
        check(kc, base.ref(k, m, B), 3000)
    # a sample of whole FASTQ records places the bins as the equivalent FASTA sample does
    with fk.KmerCounter(k, m, 3, B, n_ranks=2, rank=0, input_format="fastq") as kc:
        owners = kc.balance_bins(fastq_bytes(base.records[:500]))
    with fk.KmerCounter(k, m, 3, B, n_ranks=2, rank=0) as kc:
        assert np.array_equal(owners, kc.balance_bins(fasta_bytes(base.records[:500])))
    assert set(owners.tolist()) == {0, 1}


# ---- 10. the CLI

def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_cli_auto_format_writes_the_oracles_files(tmp_path, base):
    k, m, B = CONFIGS[0]
    inp = tmp_path / "reads.fq"
    inp.write_bytes(base.fastq)
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("FASTKMER_CLI_")}
    env["FASTKMER_CLI_FORMAT"] = "auto"
    r = subprocess.run([fk.CLI_PATH, str(k), str(m), "3", str(B), "0", "0", str(inp), str(tmp_path) + "/", "fq_",
                        "1", "0", "0"], capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    tc = fk.TestConfiguration(str(inp), str(tmp_path) + "/", k, m, 3, max_b=B, prefix="fq_")
    base.ref(k, m, B).write_bins(str(tmp_path / "ref"))
    got, exp = _files(tc.outputDir), _files(tmp_path / "ref")
    assert sorted(got) == sorted(exp) and len(got) > 32
    assert not [f for f in exp if got[f] != exp[f]]
