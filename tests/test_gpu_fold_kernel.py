"""The fold kernels (k_fold_sc, k_fold_compact) on synthetic staged pieces, through the C-ABI.

KmerCounter.debug_count_pieces folds the pieces named by fold_mask with the job's own fold before
its own count; debug_staged_piece reads the folded piece back.  The fold packs a super-cell's cells
greedily into batches of at most 1024 keys, copies a larger cell through, writes ceil(m / wmax)
entries per k-mer of multiplicity m and counting-sorts them by cell, so the shapes here sit on the
batch edges: cells of 1024 and 1025 keys, neighbours summing to 1024 and 1025, every cell of a
super-cell non-empty, an all-empty super-cell between full ones, 2^5 and 2^6 cells per super-cell.
Checked entry by entry on the folded piece first (the multiset of (k-mer, summed weight) per cell,
the weight cap, the entries per k-mer, the cell offsets, fold_stats), then on the job's count over
the folded and an unfolded piece, bit-exact against np.unique.
"""
import numpy as np
import pytest

import fastkmer_amd as fk
import staged_util as su

pytestmark = pytest.mark.gpu
FOLD_HC = 1024


def fold_cells(rng, k, F, F2, weighted, wmax):
    """The shapes, one per super-cell (2^F2 cells each); weights 1..wmax when weighted."""
    ncs = 1 << F2

    def cell(sc, i, n, d, heavy=False):
        km = su.distinct_kmers(rng, k, F, sc * ncs + i, d)
        e, w = su.cell_entries(rng, km, n, False, heavy)
        if weighted:
            w = rng.integers(1, wmax + 1, n)
            w[0] = wmax
            w[-1] = 1
        return su.piece(0, e, w, k)

    cells = [cell(0, 0, 1024, 300), cell(0, 1, 1025, 300),              # a full batch, then a cell copied through
             cell(1, 3, 512, 100), cell(1, 4, 512, 512),                # two cells of exactly 1024 together
             cell(2, 0, 512, 200), cell(2, 1, 513, 200),                # 1025: two batches
             cell(3, 5, 1, 1), cell(3, 6, 1023, 400, True), cell(3, 7, 1, 1),   # 1 + 1023 = 1024, then 1
             cell(4, ncs - 1, 2000, 50), cell(4, 0, 700, 10), cell(4, 1, 700, 700)]  # a large cell at the end
    cells += [cell(5, i, 16, 5) for i in range(ncs)]                    # every cell non-empty
    cells += [cell(7, i, 16, 16) for i in range(ncs)]                   # super-cell 6 all empty, between full ones
    cells += [cell(8, 2, 1024, 1)]                                      # one k-mer in 1024 entries (of weight wmax)
    last_sc = (1 << (F - F2)) - 1
    cells += [cell(last_sc, ncs - 1, 900, 30), cell(last_sc, ncs - 2, 300, 300)]
    if weighted:
        b, km, w = cells[-3]
        cells[-3] = (b, km, np.full(len(w), wmax))
    return cells


def per_cell(keys, cb, k):
    """{cell: {k-mer: [weights]}} of a staged piece of weighted keys."""
    km, w = su.split_weighted(keys, k)
    out = {}
    for g in np.nonzero(np.diff(cb.astype(np.int64)))[0].tolist():
        d = {}
        for x, y in zip(km[int(cb[g]):int(cb[g + 1])].tolist(), w[int(cb[g]):int(cb[g + 1])].tolist()):
            d.setdefault(x, []).append(y)
        out[g] = d
    return out


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("wmax", [15, 2, 1])
@pytest.mark.parametrize("k,F", [(16, 13), (28, 13), (28, 14), (30, 14), (30, 13)])
def test_fold_entry_by_entry_then_the_count(monkeypatch, k, F, wmax, weighted):
    monkeypatch.setenv("FASTKMER_DEBUG_FOLD_WMAX", str(wmax))
    F2 = 5 if F == 13 else 6
    rng = np.random.default_rng(1000 * k + 10 * F + wmax)
    cells = fold_cells(rng, k, F, F2, weighted, wmax)
    folded_in = su.concat_pieces(cells, k)
    # a second piece, not folded: some of the same k-mers and new ones
    b, km, w = folded_in
    pick = rng.choice(len(b), 3000, replace=False)
    other = su.concat_pieces([(b[pick], km[pick], w[pick]), su.one_cell(rng, k, F, 40, 600, 600, weighted)], k)
    pieces = [folded_in, other]
    with fk.KmerCounter(k, 10, 3, 1) as kc:
        keys, counts = su.layout(pieces, k, F, 1, rng, weighted)
        kc.debug_count_pieces(F, keys, counts, weighted, fold_mask=1)
        st, fs = kc.stats(), kc.fold_stats()
        assert st["fine_bits"] == F and st["pieces_counted"] == 2 and fs["pieces_folded"] == 1  # the fold ran
        # ---- the folded piece, entry by entry
        fkeys, fcb = kc.debug_staged_piece(0)
        raw_cb = np.concatenate([[0], np.cumsum(counts[0].astype(np.int64))])
        raw = per_cell(keys[0], raw_cb, k)  # unweighted keys: weight 1
        got = per_cell(fkeys, fcb, k)
        assert fcb[0] == 0 and np.all(np.diff(fcb.astype(np.int64)) >= 0) and int(fcb[-1]) == len(fkeys)
        assert set(got) == set(raw)
        for g, want in raw.items():
            n_raw = sum(len(v) for v in want.values())
            have = got[g]
            assert {x: sum(v) for x, v in have.items()} == {x: sum(v) for x, v in want.items()}, f"cell {g}"
            if n_raw > FOLD_HC:  # copied through
                assert {x: sorted(v) for x, v in have.items()} == {x: sorted(v) for x, v in want.items()}, f"cell {g}"
                continue
            for x, v in have.items():
                mult = sum(want[x])
                assert max(v) <= wmax and len(v) == -(-mult // wmax), f"cell {g}: {mult} occurrences in {v}"
                assert sorted(v) == sorted([wmax] * (mult // wmax) + ([mult % wmax] if mult % wmax else []))
        assert fs["entries_in"] == len(keys[0]) and fs["entries_out"] == len(fkeys)
        if wmax > 1:
            assert fs["entries_out"] < fs["entries_in"]
        ukeys, ucb = kc.debug_staged_piece(1)  # the other piece is as given
        assert np.array_equal(ukeys, keys[1]) and np.array_equal(np.diff(ucb.astype(np.int64)), counts[1].astype(np.int64))
        # ---- the job's count over the folded and the unfolded piece
        su.assert_counted(kc, su.reference(pieces, k, 1))


@pytest.mark.parametrize("mask", [0b11111, 0b10101, 0b01010])
def test_fold_of_several_pieces(mask):
    k, F = 28, 13
    rng = np.random.default_rng(mask)
    cells = fold_cells(rng, k, F, 5, False, 15)
    pieces = su.deal(rng, cells, 5, k)
    with fk.KmerCounter(k, 10, 3, 1) as kc:
        keys, counts = su.layout(pieces, k, F, 1, rng)
        kc.debug_count_pieces(F, keys, counts, False, fold_mask=mask)
        fs = kc.fold_stats()
        nf = bin(mask).count("1")
        assert fs["pieces_folded"] == nf
        assert fs["entries_in"] == sum(len(keys[p]) for p in range(5) if mask >> p & 1)
        for p in range(5):
            fkeys, fcb = kc.debug_staged_piece(p)
            raw_cb = np.concatenate([[0], np.cumsum(counts[p].astype(np.int64))])
            if not mask >> p & 1:
                assert np.array_equal(fkeys, keys[p]) and np.array_equal(fcb.astype(np.int64), raw_cb)
                continue
            raw, got = per_cell(keys[p], raw_cb, k), per_cell(fkeys, fcb, k)
            assert {g: {x: sum(v) for x, v in d.items()} for g, d in got.items()} == \
                   {g: {x: sum(v) for x, v in d.items()} for g, d in raw.items()}
        su.assert_counted(kc, su.reference(pieces, k, 1))


def test_fold_is_refused_where_it_would_grow_a_piece(monkeypatch):
    # weights above the cap in a piece to fold: ceil(m / wmax) entries per k-mer could exceed the piece
    k, F = 28, 13
    rng = np.random.default_rng(3)
    cells = [su.one_cell(rng, k, F, 8, 100, 100, True)]
    keys, counts = su.layout(cells, k, F, 1, rng, True)
    monkeypatch.setenv("FASTKMER_DEBUG_FOLD_WMAX", "2")
    with fk.KmerCounter(k, 10, 3, 1) as kc:
        with pytest.raises(fk.FastKmerError) as e:
            kc.debug_count_pieces(F, keys, counts, True, fold_mask=1)
        assert e.value.code == -1
        kc.debug_count_pieces(F, keys, counts, True)
        su.assert_counted(kc, su.reference(cells, k, 1))
