"""Every k from 1 to 64: the count, then every view of the result, against the CPU oracle (needs a GPU).

One small input per k (views_util.EveryK: random, repeated, N / lower-case / CR reads, poly-A and poly-T, a
self-complementary repeat, reads of k, k - 1 and 0 bases) under m(k) = min(k, 1 + 7k mod 15), which walks
m = 1..15 with m = k and m = 1 among them, and B = (1, 64, 2048)[k mod 3].  k = 64 (128 - 2k = 0), k <= 4 (a
handful of keys, every bucket heavy), k < 21 (2k bounds the cell bits) and the last widths with a weight nibble
(29, 30) are all in the sweep.  Everything is exact and comes from oracle.OracleResult, numpy or plain Python."""
import numpy as np
import pytest

import fastkmer_amd as fk
import views_util as vu
from query_util import pack
from test_gpu_compare import check_joined_bin, check_matrix
from test_gpu_parity import assert_same_as_oracle
from test_gpu_reads import check_batch, csr
from test_gpu_spectrum import _files as files, check_bin, check_spectrum, sorted_bin

pytestmark = pytest.mark.gpu

MAX = fk.MAX_COUNT


def run_counter(fasta, e, **kw):
    kc = fk.KmerCounter(e.k, e.m, 3, e.B, **kw)
    kc.ingest(fasta)
    kc.finish()
    return kc


def check_ranges(kc, e):
    full = np.nonzero(e.job.sizes(1, MAX))[0]
    some = full[np.linspace(0, len(full) - 1, min(len(full), 64)).astype(np.int64)]  # every bin, or 64 across them
    for lo, hi in ((1, 1), (2, MAX), (e.top, e.top)):
        want = e.job.sizes(lo, hi)
        got = kc.bin_sizes(min_count=lo, max_count=None if hi == MAX else hi)
        assert np.array_equal(got, want), f"[{lo}, {hi}]: bins {np.nonzero(got != want)[0][:5]} differ"
        for b in some.tolist():
            assert check_bin(kc, e.job, b, lo, hi) == want[b]
    assert e.job.sizes(e.top, e.top).sum() >= 1


def check_lookups(kc, e):
    hi, lo, want, want_bin = e.probes()
    kw = 2 if e.k > 32 else 1
    keys = pack(hi, lo, e.k)
    assert keys.size == len(lo) * kw
    got, bins = kc.query(keys, return_bins=True)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} counts differ, e.g. probe {bad[:5]}: {got[bad[:5]]} != {want[bad[:5]]}"
    bad = np.nonzero(bins != want_bin)[0]
    assert len(bad) == 0, f"{len(bad)} bins differ, e.g. probe {bad[:5]}: {bins[bad[:5]]} != {want_bin[bad[:5]]}"
    assert np.array_equal(kc.query(keys), want)
    # query_sequence over the joined reads: N, lower case and CR inside
    seq = b"".join(e.reads)
    bases, offsets = csr([seq])
    want_c, _ = vu.window_counts(e.tab, bases, offsets, e.k)
    got = kc.query_sequence(seq)
    assert len(got) == len(seq) - e.k + 1 and np.array_equal(got, want_c[:len(got)])


def check_profiles(kc, e):
    b1, o1 = fk.reads_csr(e.fasta)
    assert len(o1) - 1 == len(e.reads) and bytes(b1) == b"".join(e.reads)
    b2, o2 = csr(e.profile_reads())
    bases, offsets = np.concatenate([b1, b2]), np.concatenate([o1, o2[1:] + o1[-1]])
    want_c, want_v = check_batch(kc, e.tab, bases, offsets, rng=(2, e.top))
    own = slice(0, int(o1[-1]))
    assert int(want_v[own].sum()) == e.ref.total_kmers and want_c[own][want_v[own] != 0].min() >= 1


def check_text(kc, e, d):
    kc.write_bins(str(d))
    got, want = files(d), vu.table_texts(e.tab, e.k)
    assert sorted(got) == sorted(want)
    bad = [f for f in want if got[f] != want[f]]
    assert not bad, f"{len(bad)} bin files differ from the oracle's text, e.g. {bad[:3]}"


def check_comparison(ka, kb, e):
    p = e.pair
    for rows, cols in ((2, 2), (70, 5), (256, 256)):
        check_matrix(ka, kb, p, rows, cols)  # ... and the transposed call
    for side, (x, y) in enumerate(((ka, kb), (kb, ka))):
        full = np.nonzero(p.sizes(side, (1, MAX, 0, MAX)))[0]
        some = sorted({int(full[0]), int(full[len(full) // 2]), int(full[-1])})
        for rg in ((1, MAX, 1, MAX), (1, MAX, 0, 0), (2, 3, 1, 1)):  # both, A minus B, a range on either side
            want = p.sizes(side, rg)
            assert np.array_equal(x.bin_sizes_joined(y, *rg), want), (side, rg)
            for b in some:
                assert check_joined_bin(x, y, p, side, b, rg) == want[b]


def check_bins(kc, e, ordered=True):
    """bin_sizes and get_bin of every bin against the oracle's table (as sets for the table count's order)."""
    t, kw = e.tab, 2 if e.k > 32 else 1
    assert np.array_equal(kc.bin_sizes(), e.job.sizes(1, MAX))
    keys = pack(t.hi, t.lo, e.k)
    for a, b in zip(t.first, t.last):
        got_k, got_c = kc.get_bin(int(t.bin[a]))
        if not ordered:
            got_k, got_c = sorted_bin(got_k, got_c, e.k)
        assert np.array_equal(got_k, keys[a * kw:(b + 1) * kw]), f"keys differ in bin {t.bin[a]}"
        assert np.array_equal(got_c, t.count[a:b + 1]), f"counts differ in bin {t.bin[a]}"


def check_copy(kc, e, path=None):
    """A copy of the result (imported or loaded) answers as the oracle says."""
    check_bins(kc, e)
    check_spectrum(kc, e.job, 64)
    got, bins = kc.query(pack(e.tab.hi, e.tab.lo, e.k), return_bins=True)
    assert np.array_equal(got, e.tab.count) and np.array_equal(bins, e.tab.bin)
    st = kc.stats()
    assert st["distinct"] == e.ref.distinct and st["kmers"] == e.ref.total_kmers
    if path is not None:
        info = fk.db_info(path)
        assert (info["k"], info["m"], info["bins"]) == (e.k, e.m, e.nbins)
        assert info["distinct"] == e.ref.distinct and info["kmers"] == e.ref.total_kmers


@pytest.mark.parametrize("k", range(1, 65))
def test_count_and_every_view(tmp_path, k):
    e = vu.every_k(k)
    with run_counter(e.fasta, e) as kc:
        # the count
        assert_same_as_oracle(kc, e.ref)
        assert kc.stats()["kmers"] == e.ref.total_kmers and kc.stats()["distinct"] == e.ref.distinct
        # the views
        for n in (2, 3, 1025, e.top + 1, e.top + 2):
            check_spectrum(kc, e.job, n)
        check_ranges(kc, e)
        check_lookups(kc, e)
        check_profiles(kc, e)
        check_text(kc, e, tmp_path / "bins")
        with run_counter(e.fasta2, e) as kb:
            check_comparison(kc, kb, e)
        # export -> import and save -> load
        keys, counts, sizes = kc.export_arrays()
        assert np.array_equal(keys, pack(e.tab.hi, e.tab.lo, k)) and np.array_equal(counts, e.tab.count)
        assert np.array_equal(sizes.astype(np.int64), e.ref.bin_sizes())
        with fk.KmerCounter(k, e.m, 3, e.B) as copy:
            copy.import_arrays(keys, counts, sizes)
            check_copy(copy, e)
        path = str(tmp_path / "result.fkdb")
        kc.save(path)
        with fk.KmerCounter.load(path) as copy:
            assert (copy.k, copy.m, copy.num_bins) == (k, e.m, e.nbins)
            check_copy(copy, e, path)
    # the table count: bins as sets, the spectrum, a count range, the lines of the text as sets without EOF
    with run_counter(e.fasta, e, use_ht=True) as kc:
        check_bins(kc, e, ordered=False)
        for n in (2, 64, e.top + 2):
            check_spectrum(kc, e.job, n)
        assert np.array_equal(kc.bin_sizes(min_count=2), e.job.sizes(2, MAX))
        kc.write_bins(str(tmp_path / "ht"))
        got, want = files(tmp_path / "ht"), vu.table_texts(e.tab, k, eof=False)
        assert sorted(got) == sorted(want) and not any(t.endswith(b"EOF") for t in got.values())
        bad = [f for f in want if sorted(got[f].splitlines(keepends=True)) != sorted(want[f].splitlines(keepends=True))]
        assert not bad, f"{len(bad)} table-order bin files hold other lines than the oracle's, e.g. {bad[:3]}"
