"""Per-read profiles (fk_read_counts*, fk_read_stats*) against the CPU oracle, through the C-ABI only.

A batch's expectation is made in numpy: the windows are cut from (bases, offsets) by the header's
sentences (a window exists inside one read, is valid when it holds only A/C/G/T), their keys looked up in
query_util.OracleTable, the per-read statistics taken with np.sort.  Everything is exact."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fastkmer_amd as fk
from query_util import OracleTable, U64, canonical, pack
from test_gpu_query import REP, run_counter, small_job

pytestmark = pytest.mark.gpu

T = fk.READ_TILE
CODE = np.full(256, 4, dtype=np.uint8)
CODE[list(b"ACGT")] = [0, 1, 2, 3]


def csr(reads):
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(U64)
    return bases, offsets


def windows(bases, offsets, k):
    """(valid, hi, lo): valid[p] for every base position, and the forward keys of the valid windows."""
    n = len(bases)
    code = CODE[bases]
    lens = np.diff(offsets.astype(np.int64))
    end = np.repeat(offsets[1:].astype(np.int64), lens)  # the end of the read holding p
    bad = np.concatenate([[0], np.cumsum(code > 3)])
    p = np.arange(n)
    exists = p + k <= end
    valid = exists.copy()
    valid[exists] = bad[p[exists] + k] == bad[p[exists]]
    at = p[valid]
    hi, lo = np.zeros(len(at), dtype=U64), np.zeros(len(at), dtype=U64)
    for j in range(k):
        hi = (hi << U64(2)) | (lo >> U64(62))
        lo = (lo << U64(2)) | code[at + j].astype(U64)
    if k < 64:
        hi &= U64((1 << max(2 * k - 64, 0)) - 1)
    return valid, hi, lo


def expected_counts(tab, bases, offsets, k):
    valid, hi, lo = windows(bases, offsets, k)
    counts = np.zeros(len(bases), dtype=np.uint32)
    counts[valid] = tab.expected(hi, lo, k)
    return counts, valid.astype(np.uint8)


def expected_stats(counts, valid, offsets, lo=1, hi=0xFFFFFFFF):
    out = np.zeros(len(offsets) - 1, dtype=fk.READ_STAT_DTYPE)
    for i in range(len(out)):
        a, b = int(offsets[i]), int(offsets[i + 1])
        c = np.sort(counts[a:b][valid[a:b] != 0])
        if len(c):
            out[i] = (len(c), np.count_nonzero((c >= lo) & (c <= hi)), c[0], c[(len(c) - 1) // 2], c[-1], 0,
                      c.astype(np.uint64).sum())
    return out


def check_batch(kc, tab, bases, offsets, rng=(2, 40)):
    k = kc.k
    want_c, want_v = expected_counts(tab, bases, offsets, k)
    got_c, got_v = kc.read_counts(bases, offsets, return_valid=True)
    assert got_c.dtype == np.uint32 and got_v.dtype == np.uint8
    bad = np.nonzero(got_v != want_v)[0]
    assert len(bad) == 0, f"valid differs at {bad[:8]}"
    bad = np.nonzero(got_c != want_c)[0]
    assert len(bad) == 0, f"{len(bad)} counts differ, e.g. {bad[:8]}: {got_c[bad[:8]]} != {want_c[bad[:8]]}"
    assert np.array_equal(kc.read_counts(bases, offsets), want_c)
    for lo, hi in ((1, None), rng):
        got = kc.read_stats(bases, offsets, min_count=lo, max_count=hi)
        want = expected_stats(want_c, want_v, offsets, lo, 0xFFFFFFFF if hi is None else hi)
        for f in fk.READ_STAT_DTYPE.names:
            bad = np.nonzero(got[f] != want[f])[0]
            assert len(bad) == 0, f"{f} ({lo}, {hi}) differs for reads {bad[:8]}: {got[f][bad[:8]]} != {want[f][bad[:8]]}"
    return want_c, want_v


def job_reads(fasta):
    return fasta.split(b"\n")[1::2]


def revcomp_read(r):
    return r[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def edge_reads(reads, k, seed):
    """The appended reads of the small-job batch (see the issue's list)."""
    clean = [r for r in reads if set(r) <= set(b"ACGT")]
    rng = np.random.default_rng(seed)
    out = [b"", clean[0][:k - 1], clean[1][:k], clean[2][:k + 1], b"N" * 100]
    for ch in (b"N", b"\r"):
        for pos in (0, k - 1, k, 99):
            r = bytearray(clean[3 + pos % 7])
            r[pos:pos + 1] = ch
            out.append(bytes(r))
    out.append(revcomp_read(clean[10]))
    out += [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 100)].tobytes() for _ in range(200)]
    out.append(b"".join(reads[:200]))  # 20,000 bases: several tiles, N here and there
    out.append(b"")
    return out


SMALL = [(28, 10, 2048), (32, 9, 256), (33, 9, 256), (55, 12, 8192)]


# a. the small job: its own reads and every edge the batch format has
@pytest.mark.parametrize("k,m,B", SMALL)
def test_profiles_of_the_small_job(k, m, B):
    fasta, tab = small_job(k, m, B)
    reads = job_reads(fasta)
    assert len(reads) == 3000 and len(reads[-1]) == 100
    bases, offsets = csr(reads + edge_reads(reads, k, k))
    assert len(offsets) == 3000 + 216 + 1 and len(bases) > 320_000 + 4 * k
    with run_counter(fasta, k, m, B) as kc:
        want_c, want_v = check_batch(kc, tab, bases, offsets)
        st = kc.read_stats(bases, offsets)
    own = slice(0, int(offsets[3000]))
    assert want_c[own][want_v[own] != 0].min() >= 1            # the job's own windows were counted
    assert st["windows"][3000:3005].tolist() == [0, 0, 1, 2, 0] and st["windows"][-1] == 0
    # a bad byte at pos removes the windows i <= pos < i + k of the 101 - k
    left = [101 - k - (min(pos, 100 - k) - max(0, pos - k + 1) + 1) for pos in (0, k - 1, k, 99)]
    assert st["windows"][3005:3013].tolist() == left * 2 and left[0] == 100 - k
    rc = 3013
    assert st["min"][rc] >= 1 and st["windows"][rc] == 101 - k   # the other strand finds the same k-mers
    assert (st["max"][rc + 1:rc + 201] == 0).mean() > 0.9         # random reads are absent
    assert st["windows"][rc + 201] > 19_000 - 200 * k


# b. read ends around the kernel's tile edges, and the host forms' chunking
def test_read_ends_at_tile_edges_and_small_chunks(monkeypatch):
    k, m, B = 28, 10, 2048
    fasta, tab = small_job(k, m, B)
    src = b"".join(r for r in job_reads(fasta) if set(r) <= set(b"ACGT"))
    ends = [T - 1, T, T + 1, T + k - 1, 2 * T - k, 2 * T, 2 * T, 2 * T + k - 1, 3 * T + 1, 3 * T + 17]
    cuts = [0] + ends
    reads = [src[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    bases, offsets = csr(reads)
    assert offsets[1:].tolist() == ends
    with run_counter(fasta, k, m, B) as kc:
        want_c, want_v = check_batch(kc, tab, bases, offsets)
        assert want_v.sum() == sum(max(len(r) - k + 1, 0) for r in reads)
        want_s = kc.read_stats(bases, offsets, min_count=2, max_count=40)
        for chunk in ("1000", "1"):
            monkeypatch.setenv("FASTKMER_QUERY_CHUNK", chunk)
            c, v = kc.read_counts(bases, offsets, return_valid=True)
            assert np.array_equal(c, want_c) and np.array_equal(v, want_v), chunk
            assert np.array_equal(kc.read_stats(bases, offsets, min_count=2, max_count=40), want_s), chunk
        # a batch of empty reads, and empty reads at a chunk's first position
        monkeypatch.setenv("FASTKMER_QUERY_CHUNK", "50")
        b2, o2 = csr([b"", b"", reads[0][:130], b"", b"", reads[1], b""])
        check_batch(kc, tab, b2, o2)
        b3, o3 = csr([b"", b""])
        assert len(kc.read_counts(b3, o3)) == 0 and not kc.read_stats(b3, o3).view(np.uint8).any()
        assert len(kc.read_stats(b3[:0], o3[:1])) == 0


# c. the profile of the very text that was counted
def test_profile_of_the_counted_text_is_the_count():
    k, m, B = 28, 10, 2048
    fasta, tab = small_job(k, m, B)
    with run_counter(fasta, k, m, B) as kc:
        bases, offsets = fk.reads_csr(fasta)
        counts, valid = kc.read_counts(bases, offsets, return_valid=True)
        stats = kc.read_stats(fasta)
        kmers = kc.stats()["kmers"]
    assert int(stats["windows"].sum()) == kmers == int(valid.sum())
    assert counts[valid != 0].min() >= 1 and not counts[valid == 0].any()
    v2, hi, lo = windows(bases, offsets, k)
    assert np.array_equal(v2, valid != 0)
    _, clo = canonical(hi, lo, k)
    uniq, first, occ = np.unique(clo, return_index=True, return_counts=True)
    assert np.array_equal(counts[valid != 0][first], occ)      # as many windows carry a k-mer as its count says
    assert len(uniq) == len(tab) and int(stats["sum"].sum()) == int((occ.astype(np.int64) ** 2).sum())


def _against_query(kc, reads):
    """read_counts over reads equals query on the same windows' keys (query is checked against the oracle)."""
    k = kc.k
    bases, offsets = csr(reads)
    valid, hi, lo = windows(bases, offsets, k)
    want = np.zeros(len(bases), dtype=np.uint32)
    want[valid] = kc.query(pack(hi, lo, k))
    got, v = kc.read_counts(bases, offsets, return_valid=True)
    assert np.array_equal(v != 0, valid) and np.array_equal(got, want)
    return got[valid]


@functools.lru_cache(maxsize=None)
def heavy_fasta(k):
    return fk.synth_fasta(60_000, 100, 3_000_000_000, seed=0xC1 + k) + REP  # test_gpu_query.heavy_job's input


# d. heavy buckets split into sub-buckets, and a result counted from staged pieces
def test_profiles_in_split_heavy_buckets(monkeypatch):
    k, m = 28, 10
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2600")
    fasta = heavy_fasta(k)
    with run_counter(fasta, k, m, 16) as kc:
        st = kc.stats()
        assert st["split_buckets"] > 100 and st["sub_buckets"] > st["split_buckets"], st
        reads = job_reads(fasta)
        got = _against_query(kc, reads[:3000] + reads[-3000:])
        assert got.min() >= 1 and got.max() >= 3000            # the repeats' k-mers


def test_profiles_after_staged_pieces(monkeypatch):
    import torch
    k, m = 28, 10
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2600")
    monkeypatch.setenv("FASTKMER_INGEST_SEG", str(262144))
    monkeypatch.setenv("FASTKMER_PIECE_BYTES", str(524288))
    fasta = heavy_fasta(k)
    host = torch.frombuffer(bytearray(fasta), dtype=torch.uint8).pin_memory()
    with fk.KmerCounter(k, m, 3, 16) as kc:
        kc.ingest_ptr(host.data_ptr(), host.numel())
        kc.finish()
        assert kc.stats()["pieces_counted"] == 4
        reads = job_reads(fasta)
        assert _against_query(kc, reads[:3000] + reads[-3000:]).min() >= 1


# e. two ranks: valid agrees, the counts sum, the statistics come from the sum
def test_profiles_on_two_exchanging_ranks():
    import torch
    from test_gpu_comm import record_shards, run_local_job
    k, m, B = 28, 10, 2048
    fasta, tab = small_job(k, m, B)
    reads = job_reads(fasta)
    bases, offsets = csr(reads[:500] + edge_reads(reads, k, 5)[:30])
    with run_counter(fasta, k, m, B) as one:
        want_c, want_v = one.read_counts(bases, offsets, return_valid=True)
        want_s = one.read_stats(bases, offsets, min_count=2, max_count=9)
    ctxs = run_local_job(record_shards(fasta, 2), k, m, 3, B)
    try:
        got = [kc.read_counts(bases, offsets, return_valid=True) for kc in ctxs]
        assert np.array_equal(got[0][1], want_v) and np.array_equal(got[1][1], want_v)
        assert got[0][0].any() and got[1][0].any()
        total = got[0][0] + got[1][0]
        assert np.array_equal(total, want_c)
        d_c, d_v = torch.from_numpy(total.view(np.int32)).cuda(), torch.from_numpy(want_v).cuda()
        d_o = torch.from_numpy(offsets.view(np.int64)).cuda()
        d_s = torch.full((len(offsets) - 1, 32), 0x55, dtype=torch.uint8, device="cuda")
        ctxs[1].read_stats_of_counts_ptr(d_c.data_ptr(), d_v.data_ptr(), d_o.data_ptr(), len(offsets) - 1,
                                         d_s.data_ptr(), min_count=2, max_count=9)
        torch.cuda.synchronize()
        assert np.array_equal(d_s.cpu().numpy().reshape(-1).view(fk.READ_STAT_DTYPE), want_s)
        for kc in ctxs:
            with pytest.raises(fk.FastKmerError) as e:
                kc.read_stats(bases, offsets)
            assert e.value.code == -1 and "fk_read_stats_of_counts_device" in str(e.value)
            with pytest.raises(fk.FastKmerError) as e:
                kc.read_stats_ptr(d_c.data_ptr(), d_o.data_ptr(), 1, d_c.data_ptr(), 5, d_s.data_ptr())
            assert e.value.code == -1
    finally:
        for kc in ctxs:
            kc.close()


# f. states, configuration and arguments
def test_profile_states_and_arguments():
    import torch
    k, m, B = 28, 10, 2048
    fasta, tab = small_job(k, m, B)
    bases, offsets = csr(job_reads(fasta)[:50])
    want = expected_counts(tab, bases, offsets, k)[0]

    def refused(kc, code):
        d = torch.zeros(len(bases), dtype=torch.int64, device="cuda")
        for call in (lambda: kc.read_counts(bases, offsets), lambda: kc.read_stats(bases, offsets),
                     lambda: kc.read_counts_ptr(d.data_ptr(), d.data_ptr(), 1, d.data_ptr()),
                     lambda: kc.read_stats_ptr(d.data_ptr(), d.data_ptr(), 1, d.data_ptr(), 40, d.data_ptr())):
            with pytest.raises(fk.FastKmerError) as e:
                call()
            assert e.value.code == code
        torch.cuda.synchronize()
        assert not d.any()  # nothing was queued

    with fk.KmerCounter(k, m, 3, B) as kc:
        refused(kc, -2)  # FK_E_STATE: nothing counted yet
        kc.ingest(fasta)
        refused(kc, -2)
        kc.finish()
        assert np.array_equal(kc.read_counts(bases, offsets), want)
        for bad in (dict(min_count=0), dict(min_count=5, max_count=4)):
            with pytest.raises(fk.FastKmerError) as e:
                kc.read_stats(bases, offsets, **bad)
            assert e.value.code == -1
        for o in (np.array([0, 100, 90, len(bases)], dtype=U64), np.array([1, 100, len(bases)], dtype=U64)):
            for call in (lambda: kc.read_counts(bases, o), lambda: kc.read_stats(bases, o)):
                with pytest.raises(fk.FastKmerError) as e:
                    call()
                assert e.value.code == -1 and "offsets" in str(e.value)
        kc.ingest_chunk(fasta[:114 * 10], last=False)  # a new job's first ingest drops the result
        refused(kc, -2)
        kc.ingest_chunk(fasta[114 * 10:], last=True)
        kc.finish()
        assert np.array_equal(kc.read_counts(bases, offsets), want)
    with run_counter(fasta, k, m, B, use_ht=True) as kc:
        refused(kc, -1)  # FK_E_INVALID: table order cannot be searched
        assert "use_ht" in str(fk.lib().fk_last_error())


# g. profiles beside the other readers of the result
def test_profiles_beside_get_bin_and_write_bins(tmp_path):
    k, m, B = 28, 10, 2048
    fasta, tab = small_job(k, m, B)
    bases, offsets = csr(job_reads(fasta)[:300])
    with run_counter(fasta, k, m, B) as kc:
        before = kc.read_counts(bases, offsets, return_valid=True), kc.read_stats(bases, offsets)
        assert np.array_equal(before[0][0], expected_counts(tab, bases, offsets, k)[0])
        sizes = kc.bin_sizes()
        kc.get_bin(int(np.nonzero(sizes)[0][0]))
        kc.write_bins(str(tmp_path / "bins"))  # materialises the dense result
        after = kc.read_counts(bases, offsets, return_valid=True), kc.read_stats(bases, offsets)
    assert np.array_equal(after[0][0], before[0][0]) and np.array_equal(after[0][1], before[0][1])
    assert np.array_equal(after[1], before[1])


# h. the device forms on the caller's stream
def test_device_forms_on_the_callers_stream():
    import torch
    k, m, B = 55, 12, 8192
    fasta, tab = small_job(k, m, B)
    reads = job_reads(fasta)
    bases, offsets = csr(reads[:400] + edge_reads(reads, k, 9)[:40])
    n, nr = len(bases), len(offsets) - 1
    for stream in (None, torch.cuda.Stream()):
        with run_counter(fasta, k, m, B) as kc:  # closed before the stream goes away
            want_c, want_v = kc.read_counts(bases, offsets, return_valid=True)
            want_s = kc.read_stats(bases, offsets, min_count=2)
            with torch.cuda.stream(stream):
                kc.set_stream(torch.cuda.current_stream().cuda_stream)
                d_b = torch.from_numpy(bases).cuda()
                d_o = torch.from_numpy(offsets.view(np.int64)).cuda()
                d_c = torch.full((n,), -7, dtype=torch.int32, device="cuda")
                d_c2 = torch.full((n,), -7, dtype=torch.int32, device="cuda")
                d_v = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
                d_s = torch.full((2, nr, 32), 0x55, dtype=torch.uint8, device="cuda")
                scratch = torch.empty(fk.read_stats_scratch_bytes(n), dtype=torch.uint8, device="cuda")
                kc.read_counts_ptr(d_b.data_ptr(), d_o.data_ptr(), nr, d_c.data_ptr(), d_v.data_ptr())
                kc.read_counts_ptr(d_b.data_ptr(), d_o.data_ptr(), nr, d_c2.data_ptr())
                kc.read_stats_ptr(d_b.data_ptr(), d_o.data_ptr(), nr, scratch.data_ptr(), scratch.numel(),
                                  d_s[0].data_ptr(), min_count=2)
                kc.read_stats_of_counts_ptr(d_c.data_ptr(), 0, d_o.data_ptr(), nr, d_s[1].data_ptr(), min_count=2)
                kc.read_counts_ptr(0, 0, 0, 0)
                torch.cuda.current_stream().synchronize()
            assert np.array_equal(d_c.cpu().numpy().view(np.uint32), want_c)
            assert np.array_equal(d_c2.cpu().numpy().view(np.uint32), want_c)
            assert np.array_equal(d_v.cpu().numpy(), want_v)
            got = d_s.cpu().numpy().reshape(2, -1).view(fk.READ_STAT_DTYPE)
            assert np.array_equal(got[0], want_s)
            # without valid flags every existing window counts, the invalid ones with count 0
            every = expected_stats(want_c, expected_counts(tab, np.full(n, 65, dtype=np.uint8), offsets, k)[1], offsets, 2)
            assert np.array_equal(got[1], every)
            assert np.array_equal(kc.read_counts(bases, offsets), want_c)  # the host forms run on that stream too


# i. the command-line driver
def test_cli_read_stats(tmp_path):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "short_reads_k28.fa")
    with open(golden, "rb") as f:
        fasta = f.read()
    base = {k: v for k, v in os.environ.items() if not k.startswith("FASTKMER_CLI_")}
    args = ["28", "10", "3", "64", "0", "0", golden, str(tmp_path) + "/", "p_", "0", "0", "0"]
    r = subprocess.run([fk.CLI_PATH] + args, capture_output=True, text=True,
                       env=dict(base, FASTKMER_CLI_READS=golden, FASTKMER_CLI_MIN_COUNT="2", FASTKMER_CLI_MAX_COUNT="5"))
    assert r.returncode == 0, r.stderr
    with run_counter(fasta, 28, 10, 64) as kc:
        bases, offsets = fk.reads_csr(fasta)
        st = kc.read_stats(fasta, min_count=2, max_count=5)
    assert len(st) > 10 and st["hits"].any() and (st["hits"] < st["windows"]).any()
    want = "".join(f"{i}\t{int(offsets[i + 1] - offsets[i])}\t{s['windows']}\t{s['hits']}\t{s['min']}\t{s['median']}"
                   f"\t{s['max']}\t{s['sum']}\n" for i, s in enumerate(st))
    assert (tmp_path / "p_k28_m10_x3_b64_s0" / "read_stats.tsv").read_text() == want
    assert "read_stats.tsv" in r.stdout
    ht = args[:4] + ["1"] + args[5:]
    r = subprocess.run([fk.CLI_PATH] + ht, capture_output=True, text=True, env=dict(base, FASTKMER_CLI_READS=golden))
    assert r.returncode == 2 and "usage" in r.stderr and "FASTKMER_CLI_READS" in r.stderr
