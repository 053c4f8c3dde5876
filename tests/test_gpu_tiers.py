"""The staged count's tiers on synthetic staged pieces, through the C-ABI.

KmerCounter.debug_count_pieces hands the job's own staged count -- the greedy bucket cut, the wave
tier, the mid tier (key ranges / whole on the 512-key table / the 1024-key wave), the split with its
second cut, the block kernel or LDS sort, the big table and the streaming path -- pieces built in
numpy (tests/staged_util.py), so that bucket sizes, distinct counts and u16 edges that a FASTA input
reaches only by luck are hit exactly.  Every result is compared bit-exactly with np.unique (weights
summed in int64), and every test first asserts through stats() / debug_tier_stats() that the tier
it aims at took a bucket.  With F = 9 a bin has 512 cells and the greedy cut starts a bucket at every
8th cell, so a cell at a multiple of 8 followed by empty cells is a bucket of its own.
"""
import functools

import numpy as np
import pytest

import fastkmer_amd as fk
import oracle
import staged_util as su
from test_gpu_parity import assert_same_as_oracle

pytestmark = pytest.mark.gpu
F9 = 9
PIECES = [1, 2, 5]
WEIGHTED = [False, True]


def count(kc, rng, F, cells, n_pieces=1, weighted=False, fold_mask=0, order="random", modes=su.MODES):
    """The cells dealt over n_pieces, laid out and counted; returns (stats, census, reference)."""
    pieces = su.deal(rng, cells, n_pieces, kc.k, modes)
    keys, counts = su.layout(pieces, kc.k, F, kc.num_bins, rng, weighted, order)
    kc.debug_count_pieces(F, keys, counts, weighted, fold_mask)
    st = kc.stats()
    assert st["pieces_counted"] == n_pieces and st["fine_bits"] == F
    return st, kc.debug_tier_stats(), su.reference(pieces, kc.k, kc.num_bins)


def check(kc, ref):
    su.assert_counted(kc, ref, ordered=not kc.use_ht)


def mixed_weights(cells, weighted):
    if weighted:
        w = np.concatenate([c[2] for c in cells])
        assert w.min() == 1 and w.max() == 15


# ---- the wave tier through the driver

@pytest.mark.parametrize("use_ht", [False, True])
@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("n_pieces", PIECES)
def test_wave_tier(n_pieces, weighted, use_ht):
    k, m, B = 28, 10, 4
    rng = np.random.default_rng(100 + n_pieces + 10 * weighted)
    c = functools.partial(su.one_cell, rng, k, F9, weighted=weighted, m=m, B=B)
    cells = [c(0, 1, 1, bn=0),       # the first cell of the first bin
             c(8, 64, 40, bn=0), c(16, 65, 65, bn=0), c(24, 511, 300, bn=0, heavy=True), c(32, 512, 512, bn=0),
             c(40, 512, 1, bn=0),    # one k-mer under mixed weights
             c(56, 300, 200, bn=0), c(58, 300, 200, bn=0),  # cell 57 empty, 58 starts a bucket (300 + 300 > 512)
             c(8, 100, 60, bn=2), c(9, 100, 60, bn=2), c(10, 100, 60, bn=2),  # one bucket of three cells
             c(511, 65, 30, bn=3)]   # the last cell of the last bin; bin 1 stays empty
    mixed_weights(cells, weighted)
    with fk.KmerCounter(k, m, 3, B, use_ht) as kc:
        st, ts, ref = count(kc, rng, F9, cells, n_pieces, weighted)
        assert st["block_buckets"] == 0 and st["big_buckets"] == 0 and st["buckets"] >= 10  # the wave tier took all
        assert ts == {"nmidfb": 0, "nfbB": 0, "nfbG": 0, "nlarge": 0, "mid_mode": None}
        assert len(ref[1][0]) == 0 and kc.bin_sizes()[1] == 0
        check(kc, ref)


# ---- wave / mid / big boundaries

@pytest.mark.parametrize("mid_parts", ["0", "1", "2"])
@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("n,tier", [(512, "wave"), (513, "block"), (1024, "block"), (1025, "big")])
def test_bucket_size_boundaries(monkeypatch, n, tier, weighted, mid_parts):
    monkeypatch.setenv("FASTKMER_DEBUG_MID_PARTS", mid_parts)
    k, m = 28, 10
    rng = np.random.default_rng(n + 7 * weighted)
    cells = [su.one_cell(rng, k, F9, 16, n, n // 2, weighted), su.one_cell(rng, k, F9, 40, 100, 50, weighted)]
    for n_pieces in PIECES:
        with fk.KmerCounter(k, m, 3, 1) as kc:
            st, ts, ref = count(kc, rng, F9, cells, n_pieces, weighted, modes=("last", "not_first"))
            assert st["block_buckets"] == (tier == "block") and st["big_buckets"] == (tier == "big")
            if tier == "block":
                assert ts["mid_mode"] == (None, "ranges", "whole")[int(mid_parts)]
                if mid_parts == "2":
                    assert ts["nmidfb"] == 0  # n // 2 <= 512 distinct: counted whole on the 512-key table
            if tier == "big":
                assert st["split_buckets"] + ts["nfbB"] + ts["nfbG"] == 1
            check(kc, ref)


@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("n_pieces", PIECES)
@pytest.mark.parametrize("mid_parts,n,d,heavy,handed_on", [
    ("1", 900, 301, True, True),     # key ranges: 600 copies of one k-mer and 300 more -- a range above 512 keys
    ("1", 700, 700, False, None),    # key ranges, all distinct
    ("2", 800, 600, False, True),    # whole bucket: more than 512 distinct
    ("2", 1024, 512, False, False),  # whole bucket: exactly 512 distinct of 1024
    ("0", 800, 600, False, False),   # the 1024-key wave alone
])
def test_mid_tier(monkeypatch, mid_parts, n, d, heavy, handed_on, n_pieces, weighted):
    monkeypatch.setenv("FASTKMER_DEBUG_MID_PARTS", mid_parts)
    k, m = 28, 10
    rng = np.random.default_rng(n + d + n_pieces)
    km = su.distinct_kmers(rng, k, F9, 24, d)
    if heavy:  # 600 copies of km[0], the others once
        idx = np.concatenate([np.zeros(n - (d - 1), dtype=np.int64), np.arange(1, d)])
        w = rng.integers(1, 16, n) if weighted else np.ones(n, dtype=np.int64)
        cell = su.piece(0, km[idx], w, k)
    else:
        cell = su.piece(0, *su.cell_entries(rng, km, n, weighted), k)
    cells = [cell, su.one_cell(rng, k, F9, 48, 700, 100, weighted)]
    with fk.KmerCounter(k, m, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F9, cells, n_pieces, weighted, modes=("random", "last"))
        assert st["block_buckets"] == 2 and st["big_buckets"] == 0
        assert ts["mid_mode"] == (None, "ranges", "whole")[int(mid_parts)]
        if handed_on is True:
            assert ts["nmidfb"] >= 1
        if handed_on is False:
            assert ts["nmidfb"] == 0
        check(kc, ref)


# ---- the split

@pytest.mark.parametrize("retry", ["0", "1"])
@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("n,order,n_pieces", [(5000, "random", 1), (5000, "asc", 2), (5000, "desc", 5),
                                              (20000, "random", 5), (20000, "asc", 1), (20000, "desc", 2)])
def test_split(monkeypatch, n, order, n_pieces, weighted, retry):
    monkeypatch.setenv("FASTKMER_DEBUG_SPLIT_RETRY", retry)
    k, m = 28, 10
    rng = np.random.default_rng(n + n_pieces)
    cells = [su.one_cell(rng, k, F9, 8, n, n, weighted), su.one_cell(rng, k, F9, 64, 90, 90, weighted)]
    with fk.KmerCounter(k, m, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F9, cells, n_pieces, weighted, order=order, modes=("random", "last"))
        assert st["big_buckets"] == 1 and st["split_buckets"] == 1 and st["sub_buckets"] >= n / 512
        assert ts["nfbB"] == 0 and ts["nfbG"] == 0 and ts["nlarge"] == 0
        check(kc, ref)


@pytest.mark.parametrize("retry", ["0", "1"])
@pytest.mark.parametrize("weighted", WEIGHTED)
def test_split_kmers_differing_in_their_low_bits(monkeypatch, weighted, retry):
    # 1000 k-mers that differ only in their low 10 bits, five entries each: the splitters fall between neighbours
    monkeypatch.setenv("FASTKMER_DEBUG_SPLIT_RETRY", retry)
    k, m = 28, 10
    rng = np.random.default_rng(11)
    cells = [su.one_cell(rng, k, F9, 8, 5000, 1000, weighted, low_bits=10)]
    for n_pieces in PIECES:
        with fk.KmerCounter(k, m, 3, 1) as kc:
            st, ts, ref = count(kc, rng, F9, cells, n_pieces, weighted)
            assert st["big_buckets"] == 1 and st["split_buckets"] + ts["nfbB"] + ts["nfbG"] == 1
            assert st["split_buckets"] == 1
            check(kc, ref)


def heavy_cell(rng, k, F, cell, copies, others, weighted):
    """`copies` entries of one k-mer and `others` further k-mers once each."""
    km = su.distinct_kmers(rng, k, F, cell, others + 1)
    j = int(rng.integers(0, others + 1))
    idx = np.concatenate([np.full(copies, j), np.delete(np.arange(others + 1), j)])
    w = rng.integers(1, 16, len(idx)) if weighted else np.ones(len(idx), dtype=np.int64)
    if weighted:
        w[0], w[-1] = 15, 1
    return su.piece(0, km[idx], w, k)


# ---- what the split leaves: the block kernel, the big table, the streaming path

@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("n_pieces", PIECES)
@pytest.mark.parametrize("copies,others,where", [(1500, 500, "block"), (3000, 1000, "big"), (3000, 5000, "stream")])
def test_split_fallbacks(copies, others, where, n_pieces, weighted):
    k, m = 28, 10
    rng = np.random.default_rng(copies + others + n_pieces)
    cells = [heavy_cell(rng, k, F9, 8, copies, others, weighted), su.one_cell(rng, k, F9, 64, 90, 90, weighted)]
    with fk.KmerCounter(k, m, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F9, cells, n_pieces, weighted, modes=("random", "last"))
        assert st["big_buckets"] == 1 and st["split_buckets"] == 0
        if where == "block":
            assert (ts["nfbB"], ts["nfbG"], ts["nlarge"]) == (1, 0, 0)
        elif where == "big":
            assert (ts["nfbB"], ts["nfbG"], ts["nlarge"]) == (0, 1, 0)
        else:  # more than 4096 distinct: the big table gives up, the streaming radix path counts the bucket
            assert (ts["nfbB"], ts["nfbG"], ts["nlarge"]) == (0, 1, 1) and st["oversize_buckets"] == 1
        check(kc, ref)


# ---- the u16 edge of the big table

def total_as_weights(total):
    """`total` as entries of weight 15 and one remainder entry."""
    w = [15] * (total // 15)
    if total % 15:
        w.append(total % 15)
    return np.array(w, dtype=np.int64)


@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("total", [65534, 65535, 65536, 65549])
def test_big_table_u16_edge(total, weighted):
    # one k-mer of `total` occurrences among ~3000 k-mers of small counts in one big-tier bucket: the
    # table packs two u16 counts in a word and hands the bucket on when one would carry
    k, m = 28, 10
    rng = np.random.default_rng(total)
    km = su.distinct_kmers(rng, k, F9, 8, 3001)
    j = 1500  # neighbours on both sides in key order
    hw = total_as_weights(total) if weighted else np.ones(total, dtype=np.int64)
    if weighted:
        assert len(hw) in (4369, 4370) and hw.max() == 15
    oth = np.delete(np.arange(3001), j)
    oidx = np.concatenate([oth, rng.choice(oth, 3000)])
    ow = rng.integers(1, 4, len(oidx)) if weighted else np.ones(len(oidx), dtype=np.int64)
    cell = su.piece(0, np.concatenate([np.full(len(hw), km[j]), km[oidx]]), np.concatenate([hw, ow]), k)
    for n_pieces in (1, 5):
        with fk.KmerCounter(k, m, 3, 1) as kc:
            st, ts, ref = count(kc, rng, F9, [cell], n_pieces, weighted)
            assert st["big_buckets"] == 1 and ts["nfbG"] == 1 and ts["nfbB"] == 0  # the big table saw the bucket
            assert int(ref[0][1].max()) == total
            check(kc, ref)


@pytest.mark.parametrize("weighted", WEIGHTED)
def test_streaming_path_count_of_200000(weighted):
    k, m = 28, 10
    rng = np.random.default_rng(200000)
    km = su.distinct_kmers(rng, k, F9, 8, 5001)
    hw = total_as_weights(200000) if weighted else np.ones(200000, dtype=np.int64)
    ow = rng.integers(1, 16, 5000) if weighted else np.ones(5000, dtype=np.int64)
    cell = su.piece(0, np.concatenate([np.full(len(hw), km[2500]), np.delete(km, 2500)]), np.concatenate([hw, ow]), k)
    with fk.KmerCounter(k, m, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F9, [cell], 2, weighted)
        assert ts["nfbG"] == 1 and ts["nlarge"] == 1 and st["oversize_buckets"] == 1
        assert int(ref[0][1].max()) == 200000
        check(kc, ref)


# ---- key-width edges

def tier_cells(rng, k, F, cells, weighted, top=None):
    """A wave, a mid, a split, a block-fallback and a streaming bucket in the given cells."""
    c = functools.partial(su.one_cell, rng, k, F, weighted=weighted)
    out = [c(cells[0], 300, 200), c(cells[1], 800, 600), c(cells[2], 5000, 5000),
           heavy_cell(rng, k, F, cells[3], 1500, 500, weighted), heavy_cell(rng, k, F, cells[4], 3000, 5000, weighted)]
    if top is not None:
        out.append(top)
    return out


def assert_all_tiers(st, ts):
    assert st["block_buckets"] >= 1 and st["split_buckets"] >= 1 and ts["nfbB"] >= 1 and ts["nlarge"] >= 1


@pytest.mark.parametrize("n_pieces", [1, 5])
def test_k30_weight_in_the_top_nibble(n_pieces):
    k, m = 30, 10
    rng = np.random.default_rng(30)
    top_cell = (1 << F9) - 1  # k-mers whose top bits are all set, under weight 15 (the word's top nibble holds 14)
    km = su.distinct_kmers(rng, k, F9, top_cell, 400)
    km = km[km != np.uint64((1 << 60) - 1)]  # all T under weight 15 would be the empty-slot marker
    top = su.piece(0, np.concatenate([km, km[:100]]), 15, k)
    cells = tier_cells(rng, k, F9, [8, 16, 24, 32, 40], True, top)
    with fk.KmerCounter(k, m, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F9, cells, n_pieces, True)
        assert_all_tiers(st, ts)
        check(kc, ref)


@pytest.mark.parametrize("k", [31, 32])
@pytest.mark.parametrize("n_pieces", [1, 5])
def test_k31_k32_unweighted(k, n_pieces):
    m = 10
    rng = np.random.default_rng(k)
    top_cell = (1 << F9) - 1
    km = su.distinct_kmers(rng, k, F9, top_cell, 300)
    last = np.uint64((1 << (2 * k)) - 2)  # 0xFFFF...FE at k = 32
    km = np.unique(np.concatenate([km, [last]]))
    top = su.piece(0, np.concatenate([km, km[-50:]]), 1, k)
    cells = tier_cells(rng, k, F9, [8, 16, 24, 32, 40], False, top)
    with fk.KmerCounter(k, m, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F9, cells, n_pieces)
        assert_all_tiers(st, ts)
        assert ref[0][0][-1] == last and ref[0][1][-1] == 2
        check(kc, ref)


@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("n_pieces", [1, 5])
def test_k16(n_pieces, weighted):
    rng = np.random.default_rng(16)
    cells = tier_cells(rng, 16, F9, [0, 16, 24, 32, 511], weighted)
    with fk.KmerCounter(16, 10, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F9, cells, n_pieces, weighted)
        assert_all_tiers(st, ts)
        check(kc, ref)


@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("n_pieces", [1, 5])
def test_k5_one_kmer_per_cell(n_pieces, weighted):
    # k = 5, F = 10: 2k - F = 0, a cell is one k-mer; every tier sees buckets of a single distinct key
    k, m, F = 5, 4, 10
    rng = np.random.default_rng(5)
    sizes = {0: 1, 1: 3, 16: 512, 32: 513, 48: 1024, 64: 1025, 80: 2049, 96: 7000, 1022: 65, 1023: 300}
    cells = [su.one_cell(rng, k, F, c, n, 1, weighted) for c, n in sizes.items()]
    with fk.KmerCounter(k, m, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F, cells, n_pieces, weighted)
        assert st["block_buckets"] == 2 and st["big_buckets"] == 3
        assert st["split_buckets"] + ts["nfbB"] + ts["nfbG"] == 3 and ts["nfbB"] + ts["nfbG"] >= 1
        assert len(ref[0][0]) == len(sizes)
        check(kc, ref)


def test_refusals():
    rng = np.random.default_rng(1)
    one = np.ones(1, dtype=np.uint64)
    with fk.KmerCounter(31, 10, 3, 1) as kc:  # no weight field at k = 31
        cells = [su.one_cell(rng, 31, F9, 8, 10, 10)]
        keys, counts = su.layout(cells, 31, F9, 1, rng)
        for kw in (dict(weighted=True), dict(fold_mask=1)):
            with pytest.raises(fk.FastKmerError) as e:
                kc.debug_count_pieces(F9, keys, counts, **kw)
            assert e.value.code == -1
        kc.debug_count_pieces(F9, keys, counts)
    with fk.KmerCounter(28, 10, 3, 1) as kc:
        cells = [su.one_cell(rng, 28, F9, 8, 10, 10)]
        keys, counts = su.layout(cells, 28, F9, 1, rng)
        wrong_cell = [keys[0].copy()]
        wrong_cell[0][3] ^= np.uint64(1 << 55)
        above = [keys[0] | (one << np.uint64(60))]           # above the weight field
        field = [keys[0] | (np.uint64(3) << np.uint64(56))]  # a weight where none was announced
        for ks, kw in ((wrong_cell, {}), (above, dict(weighted=True)), (field, {})):
            with pytest.raises(fk.FastKmerError) as e:
                kc.debug_count_pieces(F9, ks, counts, **kw)
            assert e.value.code == -6, str(e.value)
        for F in (0, 16):
            with pytest.raises((fk.FastKmerError, ValueError)):
                kc.debug_count_pieces(F, keys, [np.zeros(max(1 << F, 1), dtype=np.uint64)])
        with pytest.raises(fk.FastKmerError):  # a sixth piece
            kc.debug_count_pieces(F9, keys * 6, counts * 6)
        with pytest.raises(fk.FastKmerError):  # fold_mask past the pieces
            kc.debug_count_pieces(F9, keys, counts, fold_mask=2)
        kc.debug_count_pieces(F9, keys * 5, counts * 5)
        assert kc.stats()["kmers"] == 50 and kc.stats()["distinct"] == 10
    with fk.KmerCounter(28, 10, 3, 4) as kc:  # a key in another bin than its position says
        km = su.distinct_kmers(rng, 28, F9, 8, 4, 10, 4, want_bin=1)
        keys, counts = su.layout([su.piece(2, km, 1, 28)], 28, F9, 4, rng)
        with pytest.raises(fk.FastKmerError) as e:
            kc.debug_count_pieces(F9, keys, counts)
        assert e.value.code == -6 and "bin" in str(e.value)
    with fk.KmerCounter(55, 12, 3, 1) as kc:  # 128-bit keys: four pieces, a fifth refused
        cells = [su.one_cell(rng, 55, F9, 8, 10, 10)]
        keys, counts = su.layout(cells, 55, F9, 1, rng)
        kc.debug_count_pieces(F9, keys * 4, counts * 4)
        assert kc.stats()["kmers"] == 40 and kc.stats()["distinct"] == 10
        with pytest.raises(fk.FastKmerError):
            kc.debug_count_pieces(F9, keys * 5, counts * 5)


# ---- 128-bit keys

def hi_lo_cells(rng, k, F, c_hi, c_lo):
    """300 k-mers that differ only in the hi word, and 300 that differ only in the lo word."""
    base = su.distinct_kmers(rng, k, F, c_hi, 1)[0]
    step = np.arange(1, 301, dtype=np.uint64)
    free_hi = min(2 * k - F - 64, 20)  # free low bits of the hi word
    assert free_hi >= 9
    hi_only = np.stack([(base[0] >> np.uint64(free_hi) << np.uint64(free_hi)) | step, np.full(300, base[1])], axis=1)
    base = su.distinct_kmers(rng, k, F, c_lo, 1)[0]
    lo_only = np.stack([np.full(300, base[0]), base[1] ^ step], axis=1)
    return [su.piece(0, np.concatenate([hi_only, hi_only[:150]]), 1, k),
            su.piece(0, np.concatenate([lo_only, lo_only[100:]]), 1, k)]


@pytest.mark.parametrize("k,m", [(33, 10), (55, 12), (63, 12)])
@pytest.mark.parametrize("n_pieces", [1, 2, 4])
def test_128_bit_keys(k, m, n_pieces):
    rng = np.random.default_rng(k + n_pieces)
    c = functools.partial(su.one_cell, rng, k, F9)
    cells = [c(0, 256, 200), c(8, 257, 257), c(16, 512, 300), c(24, 513, 513),
             c(32, 5000, 5000),                                    # split
             heavy_cell(rng, k, F9, 40, 1500, 500, False),         # a fallback of <= 2048 keys: the LDS sort
             heavy_cell(rng, k, F9, 48, 3000, 1000, False),        # above: the streaming path
             c(511, 100, 60)]
    if k > 36:  # at least 9 free bits in the hi word
        cells += hi_lo_cells(rng, k, F9, 64, 72)
    with fk.KmerCounter(k, m, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F9, cells, n_pieces)
        assert st["block_buckets"] == 2 + 2 * (k > 36)  # 257 and 512 (and the two 450 / 500-key cells)
        assert st["big_buckets"] == 4 and st["split_buckets"] == 2  # 513 and 5000 split
        assert (ts["nfbB"], ts["nfbG"], ts["nlarge"]) == (1, 1, 1) and ts["mid_mode"] is None
        check(kc, ref)


# ---- use_ht = 1 over the wave, mid and split tiers

@pytest.mark.parametrize("weighted", WEIGHTED)
@pytest.mark.parametrize("n_pieces", PIECES)
@pytest.mark.parametrize("mid_parts", ["1", "2"])
def test_use_ht(monkeypatch, mid_parts, n_pieces, weighted):
    monkeypatch.setenv("FASTKMER_DEBUG_MID_PARTS", mid_parts)
    k, m = 28, 10
    rng = np.random.default_rng(77 + n_pieces)
    c = functools.partial(su.one_cell, rng, k, F9, weighted=weighted)
    cells = [c(0, 400, 250), c(8, 800, 600), c(16, 1000, 400), c(24, 5000, 5000), c(32, 20000, 9000, heavy=True)]
    with fk.KmerCounter(k, m, 3, 1, use_ht=True) as kc:
        st, ts, ref = count(kc, rng, F9, cells, n_pieces, weighted)
        assert st["block_buckets"] == 2 and st["split_buckets"] >= 1 and ts["mid_mode"] == ("ranges", "whole")[int(mid_parts) - 1]
        check(kc, ref)


# ---- stale state

def test_weighted_then_unweighted_then_a_normal_job():
    k, m = 28, 10
    rng = np.random.default_rng(9)
    fasta = fk.synth_fasta(3_000, 100, 50_000, seed=0x57A1E)
    with fk.KmerCounter(k, m, 3, 1) as kc:
        st, ts, ref = count(kc, rng, F9, tier_cells(rng, k, F9, [8, 16, 24, 32, 40], True), 5, True)
        assert_all_tiers(st, ts)
        check(kc, ref)
        st, ts, ref = count(kc, rng, 13, tier_cells(rng, k, 13, [8, 64, 128, 192, 256], False), 2, False)
        assert_all_tiers(st, ts)
        check(kc, ref)
        kc.ingest(fasta)
        kc.finish()
        want = oracle.OracleResult(fasta, k, m, 1)
        assert kc.stats()["kmers"] == want.total_kmers and kc.stats()["distinct"] == want.distinct
        assert_same_as_oracle(kc, want)
        st, ts, ref = count(kc, rng, F9, tier_cells(rng, k, F9, [8, 16, 24, 32, 40], True), 1, True)
        assert_all_tiers(st, ts)
        check(kc, ref)


# ---- a seeded property test

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6000]


@pytest.mark.parametrize("seed", range(20))
def test_random_cells(seed):
    rng = np.random.default_rng(0xC0FFEE + seed)
    k, m = 28, 10
    F = [1, 5, 9, 13, 14, 15][seed % 6]
    B = 1 + seed % 2
    weighted = bool(rng.integers(0, 2))
    n_pieces = int(rng.choice([1, 2, 3, 5]))
    cells = []
    for bn in range(B):
        for cell in rng.choice(1 << F, min(1 << F, 6), replace=False).tolist():
            n = int(rng.choice(SIZES))
            if n == 0:
                continue
            kind = int(rng.integers(0, 3))  # all distinct, one k-mer, heavy-tailed
            d = (n, 1, max(1, n // 4))[kind]
            cells.append(su.one_cell(rng, k, F, cell, n, d, weighted, heavy=kind == 2, m=m, B=B, bn=bn))
    if not cells:
        cells.append(su.one_cell(rng, k, F, 0, 1, 1, weighted, m=m, B=B, bn=0))
    with fk.KmerCounter(k, m, 3, B) as kc:
        st, ts, ref = count(kc, rng, F, cells, n_pieces, weighted)
        assert st["buckets"] >= 1
        check(kc, ref)
