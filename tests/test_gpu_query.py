"""fk_query / fk_query_device / fk_query_sequence against the CPU oracle, through the C-ABI only.

Every distinct k-mer of the oracle is looked up (every other one on its reverse strand) and must give
the oracle's count and bin; keys next to the stored ones and random keys must give 0 and the bin of
fk_kmer_bin.  The inputs are the smallest that reach every layout a lookup can land in: buckets of
several cells, heavy buckets split into sub-buckets and their fallbacks, staged pieces, bins spread
over ranks (round-robin and size-aware owners).  Everything is exact; expectations are numpy arrays
(query_util.OracleTable), never dicts of k-mers."""
import functools

import numpy as np
import pytest

import fastkmer_amd as fk
import oracle
from query_util import CONFIGS, OracleTable, U64, add, is_kmer, kmer_bins, pack, revcomp

pytestmark = pytest.mark.gpu

REP = b"".join(b">q%d\n" % i + b"ACGTTGCAAGGCTTACCGATCGGATTACAGGCATCGATCGGGCTAGCTAGGCTAGCTTACGAGCTAGCATCGACTAG"
               b"CATGCATGCATCGACGTAGCATCG\n" for i in range(3_000))


def _query_all(ctxs, keys):
    """Every rank's (counts, bins) of the same keys."""
    return [kc.query(keys, return_bins=True) for kc in ctxs]


def _assert_ranks(got, want_counts, want_bins, owner):
    """The ranks' counts sum to the expectation, a rank answers only for the bins it owns, and every
    rank reports the same bins."""
    total = np.zeros(len(want_counts), dtype=np.uint64)
    for r, (counts, bins) in enumerate(got):
        assert np.array_equal(bins, want_bins), f"rank {r}: bins differ"
        mine = owner[want_bins] == r
        assert not counts[~mine].any(), f"rank {r} answers for bins it does not own"
        total += counts
    bad = np.nonzero(total != want_counts)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(total)} counts differ, e.g. query {bad[:5]}: " \
                          f"{total[bad[:5]]} != {want_counts[bad[:5]]}"


def check_lookups(ctxs, tab, k, m, B, monkeypatch, owner=None):
    """The shared checker (see the module docstring); ctxs = the job's ranks."""
    kw = 2 if k > 32 else 1
    nbins = fk.clamped_bins(m, B)
    owner = np.arange(nbins) % len(ctxs) if owner is None else np.asarray(owner)
    assert len(tab) > 0
    # 1. every distinct k-mer, the odd-indexed ones on the other strand
    qhi, qlo = tab.hi.copy(), tab.lo.copy()
    rh, rl = revcomp(tab.hi, tab.lo, k)
    qhi[1::2], qlo[1::2] = rh[1::2], rl[1::2]
    keys = pack(qhi, qlo, k)
    present = _query_all(ctxs, keys)
    _assert_ranks(present, tab.count, tab.bin, owner)
    # 2. absent keys: around every bin's key range, right after every key, and uniform random ones
    first, last = np.array(tab.first), np.array(tab.last)
    nh, nl = add(tab.hi, tab.lo, 1)
    gap = np.ones(len(tab), dtype=bool)
    gap[:-1] = (tab.hi[1:] != nh[:-1]) | (tab.lo[1:] != nl[:-1])
    rng = np.random.default_rng(k * 1000 + m)
    rnd = rng.integers(0, 2 ** 64, size=(2, 10_000), dtype=U64)
    if k < 32:
        rnd[1] &= U64((1 << (2 * k)) - 1)
    if k <= 32:
        rnd[0] = 0
    elif k < 64:
        rnd[0] &= U64((1 << (2 * k - 64)) - 1)
    below, above = add(tab.hi[first], tab.lo[first], -1), add(tab.hi[last], tab.lo[last], 1)
    ahi = np.concatenate([below[0], above[0], nh[gap], rnd[0]])
    alo = np.concatenate([below[1], above[1], nl[gap], rnd[1]])
    ok = is_kmer(ahi, alo, k)  # 0 - 1 and (4^k - 1) + 1 are no k-mers
    ahi, alo = ahi[ok], alo[ok]
    want = tab.expected(ahi, alo, k)
    absent = want == 0
    assert absent.sum() > 0.9 * len(want) and absent.sum() >= 10_000 - 10
    akeys = pack(ahi, alo, k)
    got = _query_all(ctxs, akeys)
    total = sum(c.astype(np.uint64) for c, _ in got)
    assert not total[absent].any(), f"{np.count_nonzero(total[absent])} absent keys have a count"
    assert np.array_equal(total[~absent], want[~absent])
    abins = kmer_bins(akeys, k, m, B)
    assert all(np.array_equal(b, abins) for _, b in got)
    # 3. a key that is no k-mer
    if k in (28, 55):
        bad = np.array([1 << (2 * k)], dtype=U64) if kw == 1 else np.array([1 << (2 * k - 64), 5], dtype=U64)
        mixed = np.concatenate([keys[:kw], bad, keys[kw:2 * kw]])
        for r, (c, b) in enumerate(_query_all(ctxs, mixed)):
            assert (c[1], b[1]) == (0, -1)
            assert (c[0], c[2]) == (present[r][0][0], present[r][0][1]) and (b[0], b[2]) == (tab.bin[0], tab.bin[1])
    # 4. small staging chunks change nothing
    monkeypatch.setenv("FASTKMER_QUERY_CHUNK", "1000")
    c2, b2 = ctxs[0].query(keys, return_bins=True)
    assert np.array_equal(c2, present[0][0]) and np.array_equal(b2, present[0][1])
    for n in (0, 1, 65):
        c3, b3 = ctxs[0].query(keys[:n * kw], return_bins=True)
        assert len(c3) == n and np.array_equal(c3, c2[:n]) and np.array_equal(b3, b2[:n])
        assert np.array_equal(ctxs[0].query(keys[:n * kw]), c2[:n])
    monkeypatch.delenv("FASTKMER_QUERY_CHUNK")


def run_counter(fasta, k, m, B, **kw):
    kc = fk.KmerCounter(k, m, 3, B, **kw)
    kc.ingest(fasta)
    kc.finish()
    return kc


@functools.lru_cache(maxsize=None)
def small_job(k, m, B):
    """(input, oracle table) of the multi-cell case, shared by the tests that need no other input."""
    fasta = fk.synth_fasta(3000, 100, 200_000, seed=0xA0 + k)
    ref = oracle.OracleResult(fasta, k, m, B)
    return fasta, OracleTable(ref, ref.nbins)


@functools.lru_cache(maxsize=None)
def heavy_job(k, m):
    fasta = fk.synth_fasta(60_000, 100, 3_000_000_000, seed=0xC1 + k) + REP
    ref = oracle.OracleResult(fasta, k, m, 16, threads=4)
    return fasta, OracleTable(ref, ref.nbins), ref.total_kmers


# a. buckets of several cells
@pytest.mark.parametrize("k,m,B", CONFIGS)
def test_lookups_in_multi_cell_buckets(monkeypatch, k, m, B):
    fasta, tab = small_job(k, m, B)
    with run_counter(fasta, k, m, B) as kc:
        check_lookups([kc], tab, k, m, B, monkeypatch)


# ... and, with cells of two keys (a test hook), buckets of many cells each: the lookup's c0 <= cell < c1
@pytest.mark.parametrize("k,m,B", [(21, 7, 64), (55, 12, 64)])
def test_lookups_in_buckets_of_many_cells(monkeypatch, k, m, B):
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2")
    fasta, tab = small_job(k, m, B)
    with run_counter(fasta, k, m, B) as kc:
        st = kc.stats()
        assert 4 * st["buckets"] < (kc.num_bins << st["fine_bits"]), st
        check_lookups([kc], tab, k, m, B, monkeypatch)


# b. heavy buckets: split into sub-buckets (ascending across the bucket) and their fallbacks
@pytest.mark.parametrize("k,m", [(28, 10), (55, 12)])
def test_lookups_in_split_heavy_buckets(monkeypatch, k, m):
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2600")
    fasta, tab, total = heavy_job(k, m)
    with run_counter(fasta, k, m, 16) as kc:
        st = kc.stats()
        assert st["split_buckets"] > 100 and st["kmers"] == total, st
        assert st["split_buckets"] < st["block_buckets"] + st["big_buckets"], st  # the repeats fall back
        check_lookups([kc], tab, k, m, 16, monkeypatch)


# c. a job counted from staged pieces
def test_lookups_after_staged_pieces(monkeypatch):
    import torch
    k, m = 28, 10
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2600")
    monkeypatch.setenv("FASTKMER_INGEST_SEG", str(262144))
    monkeypatch.setenv("FASTKMER_PIECE_BYTES", str(524288))
    fasta, tab, total = heavy_job(k, m)
    host = torch.frombuffer(bytearray(fasta), dtype=torch.uint8).pin_memory()
    with fk.KmerCounter(k, m, 3, 16) as kc:
        kc.ingest_ptr(host.data_ptr(), host.numel())
        kc.finish()
        st = kc.stats()
        assert st["pieces_counted"] == 4 and st["kmers"] == total, st
        check_lookups([kc], tab, k, m, 16, monkeypatch)


# d. state and configuration
def test_lookup_states_and_configuration():
    k, m, B = 28, 10, 2048
    fasta, tab = small_job(k, m, B)
    keys = pack(tab.hi[:100], tab.lo[:100], k)
    seq = fasta.split(b"\n")[1]

    def refused(kc, code):
        import torch
        d = torch.zeros(100, dtype=torch.int64, device="cuda")
        for call in (lambda: kc.query(keys), lambda: kc.query(keys, return_bins=True), lambda: kc.query_sequence(seq),
                     lambda: kc.query_ptr(d.data_ptr(), 100, d.data_ptr())):
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
        assert np.array_equal(kc.query(keys), tab.count[:100])
        kc.ingest_chunk(fasta[:114 * 10], last=False)  # a new job's first ingest drops the result
        refused(kc, -2)
        kc.ingest_chunk(fasta[114 * 10:], last=True)
        kc.finish()
        assert np.array_equal(kc.query(keys), tab.count[:100])
    with run_counter(fasta, k, m, B, use_ht=True) as kc:
        refused(kc, -1)  # FK_E_INVALID: table order cannot be searched
        assert "use_ht" in str(fk.lib().fk_last_error())
    with run_counter(b"", k, m, B) as kc:  # an empty job answers, with zeros
        c, b = kc.query(keys, return_bins=True)
        assert not c.any() and np.array_equal(b, tab.bin[:100]) and np.array_equal(b, kmer_bins(keys, k, m, B))
        assert not kc.query_sequence(seq).any() and len(kc.query_sequence(seq)) == len(seq) - k + 1


# e. ranks: round-robin owners with the library's exchange, size-aware owners by hand
def test_lookups_on_two_exchanging_ranks(monkeypatch):
    from test_gpu_comm import record_shards, run_local_job
    k, m, B = 28, 10, 2048
    fasta, tab = small_job(k, m, B)
    ctxs = run_local_job(record_shards(fasta, 2), k, m, 3, B)
    try:
        assert np.array_equal(ctxs[0].bin_owners(), np.arange(B) % 2)
        check_lookups(ctxs, tab, k, m, B, monkeypatch)
    finally:
        for kc in ctxs:
            kc.close()


def test_lookups_on_three_ranks_with_lpt_owners(monkeypatch):
    import torch
    k, m, B, G = 28, 10, 2048, 3
    fasta, tab = small_job(k, m, B)
    shards = [fasta[r * 114 * 1000:(r + 1) * 114 * 1000] for r in range(G)]
    ranks = [fk.KmerCounter(k, m, 3, B, n_ranks=G, rank=r) for r in range(G)]
    try:
        sizes = np.zeros(B, dtype=np.uint64)
        for r in range(G):
            ranks[r].ingest(shards[r])
            ranks[r].map()
            sizes += ranks[r].map_bin_kmers()
        owner = fk.lpt_owners(sizes, G)
        assert not np.array_equal(owner, np.arange(B) % G)
        rb, sends = ranks[0].record_bytes, []
        for r in range(G):
            counts = ranks[r].set_bin_owners(owner)
            buf = torch.empty(max(sum(counts), 1) * rb, dtype=torch.uint8, device="cuda")
            ranks[r].map_emit(buf.data_ptr(), max(sum(counts), 1))
            torch.cuda.synchronize()
            sends.append((buf, counts))
        for dst in range(G):
            parts = []
            for buf, counts in sends:
                off = sum(counts[:dst])
                parts.append(buf[off * rb:(off + counts[dst]) * rb])
            recv = torch.cat(parts)
            ranks[dst].reduce(recv.data_ptr(), recv.numel() // rb)
            torch.cuda.synchronize()
        check_lookups(ranks, tab, k, m, B, monkeypatch, owner=owner)
    finally:
        for kc in ranks:
            kc.close()


@pytest.fixture(scope="module")
def counted():
    """One counted job (k = 28) for the tests of the other entry points."""
    k, m, B = 28, 10, 2048
    fasta, tab = small_job(k, m, B)
    with run_counter(fasta, k, m, B) as kc:
        yield kc, fasta, tab


# f. the device form on the caller's stream
def test_query_ptr_on_the_callers_stream():
    import torch
    k, m, B = 28, 10, 2048
    fasta, tab = small_job(k, m, B)
    for stream in (None, torch.cuda.Stream()):  # torch's default stream, then a side stream
        with run_counter(fasta, k, m, B) as kc:  # closed before the stream goes away
            _check_query_ptr(kc, tab, stream)


def _check_query_ptr(kc, tab, stream):
    import torch
    k = kc.k
    qhi, qlo = tab.hi.copy(), tab.lo.copy()
    rh, rl = revcomp(tab.hi, tab.lo, k)
    qhi[::3], qlo[::3] = rh[::3], rl[::3]
    keys = np.concatenate([pack(qhi, qlo, k), np.array([1 << 62, 12345], dtype=U64)])
    want_c, want_b = kc.query(keys, return_bins=True)
    assert np.array_equal(want_c[:-2], tab.count) and want_b[-2] == -1
    n = len(keys)
    with torch.cuda.stream(stream):
        kc.set_stream(torch.cuda.current_stream().cuda_stream)
        d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
        d_counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        d_bins = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        d_only = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        kc.query_ptr(d_keys.data_ptr(), n, d_counts.data_ptr(), d_bins.data_ptr())
        kc.query_ptr(d_keys.data_ptr(), n, d_only.data_ptr())
        kc.query_ptr(0, 0, 0)
        torch.cuda.current_stream().synchronize()
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), want_c)
    assert np.array_equal(d_only.cpu().numpy().view(np.uint32), want_c)
    assert np.array_equal(d_bins.cpu().numpy(), want_b)
    # the host forms run on that stream too from now on
    assert np.array_equal(kc.query(keys), want_c)


# g. every window of a sequence
def test_query_sequence(counted, monkeypatch):
    kc, fasta, tab = counted
    k = kc.k
    reads = [r for r in fasta.split(b"\n")[1::2] if set(r) <= set(b"ACGT")][:10]
    assert len(reads) == 10

    def window_counts(read):
        keys = fk.encode_keys([read[i:i + k].decode() for i in range(len(read) - k + 1)], k)
        return tab.expected(np.zeros(len(keys), dtype=U64), keys, k)

    for read in reads:
        got = kc.query_sequence(read)
        assert got.dtype == np.uint32 and len(got) == len(read) - k + 1
        assert np.array_equal(got, window_counts(read)) and got.min() >= 1
    assert np.array_equal(kc.query_sequence(reads[0].decode()), kc.query_sequence(reads[0]))
    # an N and a lowercase base zero exactly the windows that cover them
    read = bytearray(reads[1])
    p1, p2 = 5, 60
    read[p1] = ord("N")
    read[p2] = ord(chr(read[p2]).lower())
    i = np.arange(len(read) - k + 1)
    cover = ((i <= p1) & (p1 < i + k)) | ((i <= p2) & (p2 < i + k))
    assert cover.any() and not cover.all()
    got = kc.query_sequence(bytes(read))
    assert np.array_equal(got, np.where(cover, 0, window_counts(reads[1])))
    assert not got[cover].any() and got[~cover].min() >= 1
    assert not kc.query_sequence(reads[2][:40] + b"\n" + reads[2][40:])[40 - k + 1:41].any()
    one = kc.query_sequence(reads[3][:k])
    assert len(one) == 1 and one[0] == window_counts(reads[3])[0]
    assert len(kc.query_sequence(reads[3][:k - 1])) == 0 and len(kc.query_sequence(b"")) == 0
    # the C call's buffer rules
    import ctypes
    L, n = fk.lib(), ctypes.c_size_t(99)
    assert L.fk_query_sequence(kc._h, reads[0], len(reads[0]), None, 0, ctypes.byref(n)) == 0
    assert n.value == len(reads[0]) - k + 1
    buf = np.zeros(n.value, dtype=np.uint32)
    assert L.fk_query_sequence(kc._h, reads[0], len(reads[0]), buf.ctypes.data, n.value - 1, ctypes.byref(n)) == -6
    # windows staged seven at a time
    whole = kc.query_sequence(reads[0])
    monkeypatch.setenv("FASTKMER_QUERY_CHUNK", "7")
    assert np.array_equal(kc.query_sequence(reads[0]), whole)


# h. lookups beside the other readers of the result
def test_lookups_beside_get_bin_and_write_bins(counted, tmp_path):
    kc, fasta, tab = counted
    k = kc.k
    keys = pack(*revcomp(tab.hi, tab.lo, k), k)
    before = kc.query(keys, return_bins=True)
    assert np.array_equal(before[0], tab.count) and np.array_equal(before[1], tab.bin)
    ref = oracle.OracleResult(fasta, k, kc.m, 2048)
    some = np.nonzero(ref.bin_sizes())[0][[0, 7, -1]].tolist()
    for b in some:  # gathered from the bucket-major result
        got_keys, got_counts = kc.get_bin(b)
        _, rlo, rcnt = ref.bin_arrays(b)
        assert np.array_equal(got_keys, rlo) and np.array_equal(got_counts, rcnt)
    kc.write_bins(str(tmp_path / "bins"))  # materialises the dense result
    ref.write_bins(str(tmp_path / "ref"))
    for b in some:
        assert (tmp_path / "bins" / f"bin{b}").read_bytes() == (tmp_path / "ref" / f"bin{b}").read_bytes()
    after = kc.query(keys, return_bins=True)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    for b in some:  # now read from the dense copy
        got_keys, got_counts = kc.get_bin(b)
        _, rlo, rcnt = ref.bin_arrays(b)
        assert np.array_equal(got_keys, rlo) and np.array_equal(got_counts, rcnt)
