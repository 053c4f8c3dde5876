"""The synthetic staged pieces of tests/staged_util.py and their reference, checked without a GPU:
the reference against a dict-based count, and the layout's invariants (every key in the cell and
bin its position says, the cell counts, the weight field)."""
import collections

import numpy as np
import pytest

import fastkmer_amd as fk
import staged_util as su


@pytest.fixture(scope="module", autouse=True)
def built():
    from fastkmer_amd import build
    build.build()


def to_int(row, k):
    return int(row) if k <= 32 else (int(row[0]) << 64) | int(row[1])


def make_pieces(rng, k, F, B, m, n_pieces, weighted):
    parts = []
    for bn in range(B):
        for cell in rng.choice(1 << F, min(3, 1 << F), replace=False).tolist():
            d = min(int(rng.integers(1, 40)), 1 << min(2 * k - F, 20))  # k = 5, F = 10: one k-mer per cell
            km = su.distinct_kmers(rng, k, F, cell, d, m, B, bn)
            e, w = su.cell_entries(rng, km, d + int(rng.integers(0, 60)), weighted, heavy=bool(rng.integers(0, 2)))
            parts.append(su.piece(bn, e, w, k))
    return su.spread(rng, su.concat_pieces(parts, k), n_pieces, k)


@pytest.mark.parametrize("k,m,F,B,n_pieces,weighted", [(28, 10, 9, 1, 1, False), (28, 10, 9, 3, 5, True),
                                                       (30, 10, 13, 2, 2, True), (32, 10, 5, 1, 2, False),
                                                       (5, 4, 10, 1, 2, True), (55, 12, 9, 2, 4, False),
                                                       (33, 10, 15, 1, 3, False), (63, 12, 1, 1, 2, False)])
def test_reference_and_layout(k, m, F, B, n_pieces, weighted):
    rng = np.random.default_rng(k * 100 + F)
    B = fk.clamped_bins(m, B)
    pieces = make_pieces(rng, k, F, B, m, n_pieces, weighted)
    # the reference against a dict
    want = [collections.Counter() for _ in range(B)]
    for b, km, w in pieces:
        for bn, row, wt in zip(b.tolist(), km, w.tolist()):
            want[bn][to_int(row, k)] += wt
    ref = su.reference(pieces, k, B)
    for bn in range(B):
        u, c = ref[bn]
        got = {to_int(row, k): int(n) for row, n in zip(u, c)}
        assert got == dict(want[bn]) and c.dtype == np.int64
        ints = [to_int(row, k) for row in u]
        assert ints == sorted(ints) and len(set(ints)) == len(ints)
    # the layout: every key in the cell and bin its position says, the multiset unchanged
    keys, counts = su.layout(pieces, k, F, B, rng, weighted)
    assert len(keys) == len(counts) == n_pieces
    for (b, km, w), ka, cn in zip(pieces, keys, counts):
        assert cn.dtype == np.uint64 and len(cn) == B << F and int(cn.sum()) == len(b)
        ka = su.as_kmers(ka, k)
        if weighted:
            assert not np.any(ka >> np.uint64(2 * k + 4)) if 2 * k + 4 < 64 else True
            kk, ww = su.split_weighted(ka, k)
        else:
            kk, ww = ka, np.ones(len(ka), dtype=np.int64)
        where = np.repeat(np.arange(B << F), cn.astype(np.int64))
        assert np.array_equal(su.cell_of(kk, k, F), where & ((1 << F) - 1))
        assert np.array_equal(su.bins_of(kk, k, m, B), where >> F)
        a = collections.Counter((to_int(r, k), int(x)) for r, x in zip(kk, ww))
        e = collections.Counter((to_int(r, k), int(x)) for r, x in zip(km, w))
        assert a == e
    if weighted:
        allw = np.concatenate([p[2] for p in pieces])
        assert allw.min() == 1 and allw.max() == 15


def test_layout_refuses_weights_without_a_field():
    rng = np.random.default_rng(1)
    km = su.distinct_kmers(rng, 31, 9, 3, 4)
    with pytest.raises(ValueError):
        su.layout([su.piece(0, km, 2, 31)], 31, 9, 1, rng, weighted=True)
    with pytest.raises(ValueError):
        su.layout([su.piece(0, km, 2, 31)], 31, 9, 1, rng)


def test_bins_of_matches_kmer_bin_and_low_bits():
    rng = np.random.default_rng(2)
    km = su.distinct_kmers(rng, 28, 9, 77, 50, 10, 4, want_bin=2)
    assert all(fk.kmer_bin(int(x), 28, 10, 4) == 2 for x in km)
    lo = su.distinct_kmers(rng, 28, 9, 77, 1000, low_bits=10)
    assert len(np.unique(lo >> np.uint64(10))) == 1 and len(np.unique(lo)) == 1000
