"""The model of tests/views_util.py checked against the oracle, without a GPU: its text against the golden
fixtures, the coverage its inputs and its chosen counts promise, and its read statistics against a plain
Python loop."""
import json
import os

import numpy as np
import pytest

import oracle
import views_util as vu
from conftest import GOLDEN, golden_cases
from query_util import OracleTable, U64


@pytest.fixture(scope="module", autouse=True)
def built():
    from fastkmer_amd import build
    build.build()


@pytest.mark.parametrize("name", ["short_reads_k28", "edge_bytes_k21", "k32_boundary"] +
                         [n for n, p in sorted(golden_cases().items()) if p["k"] > 32][:1])
def test_model_text_equals_the_golden_files(name):
    p = golden_cases()[name]
    with open(os.path.join(GOLDEN, name + ".fa"), "rb") as f:
        fasta = f.read()
    with open(os.path.join(GOLDEN, name + ".expected.json")) as f:
        expected = json.load(f)
    ref = oracle.OracleResult(fasta, p["k"], p["m"], p["B"], p.get("sequence_type", 0))
    tab = OracleTable(ref, ref.nbins)
    got = {f: t.decode() for f, t in vu.table_texts(tab, p["k"]).items()}
    assert got == expected and len(expected) > 0
    # the same table through the model's own Table, a range and the key round trip
    mine = vu.Table(tab.hi, tab.lo, tab.count, tab.bin)
    assert mine.first == tab.first and mine.last == tab.last
    assert vu.table_texts(mine, p["k"], 1, vu.MAX) == vu.table_texts(tab, p["k"])
    twos = vu.table_texts(mine, p["k"], 2, 2, eof=False)
    want = {f: "".join(ln + "\n" for ln in t[:-3].splitlines() if ln.endswith("\t2")) for f, t in expected.items()}
    assert {f: t.decode() for f, t in twos.items()} == {f: t for f, t in want.items() if t}
    at = mine.find(tab.hi, tab.lo, p["k"])
    assert np.array_equal(at, np.arange(len(tab)))
    assert np.array_equal(vu.oracle_bins(tab.hi, tab.lo, p["k"], p["m"], p["B"]), tab.bin)


@pytest.mark.parametrize("k", range(1, 65))
def test_every_k_input_covers_every_class(k):
    e = vu.every_k(k)  # check_classes ran on the oracle's result
    assert (e.m, e.B) == (min(k, 1 + (7 * k) % 15), (1, 64, 2048)[k % 3]) and e.nbins == e.ref.nbins
    assert e.top >= 2 * (201 - k) and len(e.tab) >= 1
    p = e.pair
    both, only_a, only_b = (p.ca > 0) & (p.cb > 0), p.cb == 0, p.ca == 0
    assert both.any() and (k < 7 or (only_a.any() and only_b.any())), "the second input shares half of the first"
    ref2 = oracle.OracleResult(e.fasta2, k, e.m, e.B)  # the second result: np.unique against the oracle's count
    want2 = OracleTable(ref2, ref2.nbins)
    for f in ("hi", "lo", "count", "bin"):
        assert np.array_equal(getattr(e.tab2, f), getattr(want2, f)), f
    assert e.tab2.first == want2.first and e.tab2.last == want2.last
    hi, lo, count, bin_ = e.probes()
    n = len(e.tab)
    assert np.array_equal(count[:n], e.tab.count) and np.array_equal(count[n:2 * n], e.tab.count)
    assert k in (32, 64) or (bin_ == -1).sum() >= (64 if k < 32 else 128) - 2 * k
    assert (count[bin_ == -1] == 0).all() and (bin_ >= -1).all() and bin_.max() < e.nbins
    texts = vu.table_texts(e.tab, k)
    assert sorted(texts) == sorted(f"bin{b}" for b in np.nonzero(e.ref.bin_sizes())[0])
    b0 = int(e.tab.bin[0])
    assert texts[f"bin{b0}"].decode() == e.ref.bin_text(b0)
    assert len(e.profile_reads()) == 52


def test_m_and_B_walk_their_ranges():
    ms = {m: [k for k in range(1, 65) if vu.m_of(k) == m] for m in range(1, 16)}
    assert all(ms.values()) and ms[1] == [1, 15, 30, 45, 60] and ms[15] == [17, 32, 47, 62]
    assert [k for k in range(1, 65) if vu.m_of(k) == k] == [1, 2, 3, 4, 5, 6, 8, 10]
    assert {vu.B_of(k) for k in range(1, 65)} == {1, 64, 2048}


@pytest.mark.parametrize("k,m,B", vu.VIEW_CONFIGS)
def test_chosen_counts_cover_every_pair_and_region(k, m, B):
    c = vu.chosen(k, m, B)  # check_coverage ran
    assert len(vu.PALETTE) == 37 == len(set(vu.PALETTE)) and vu.PALETTE == sorted(vu.PALETTE)
    assert {len(str(x)) for x in vu.PALETTE} == set(range(1, 11)), "all ten digit widths"
    for t in (c.a, c.b):
        assert set(t.count.tolist()) == set(vu.PALETTE)
        order = np.lexsort((t.lo, t.hi, t.bin))
        assert np.array_equal(order, np.arange(len(t))), "bins in order, keys ascending inside a bin"
        assert np.array_equal(vu.oracle_bins(t.hi[::50], t.lo[::50], k, m, B), t.bin[::50])
    # the expectations against plain Python over the same table
    t = c.a
    for n in (2, 1025, 65537):
        hist, tail = vu.spectrum(t.count, n)
        want = [0] * n
        for x in t.count.tolist():
            want[min(x, n - 1)] += 1
        assert hist.tolist() == want and tail == sum(x for x in t.count.tolist() if x >= n - 1)
    assert vu.spectrum(t.count, 2)[1] > 2 ** 32
    for lo, hi in vu.RANGE_PAIRS:
        sizes = vu.range_sizes(t, c.nbins, lo, hi)
        want = [0] * c.nbins
        for x, b in zip(t.count.tolist(), t.bin.tolist()):
            want[b] += lo <= x <= hi
        assert sizes.tolist() == want and sizes.sum() > 0, (lo, hi)
        keys, counts = vu.range_bin(t, k, 5, lo, hi)
        assert len(counts) == want[5] and len(keys) == want[5] * (2 if k > 32 else 1)
    for rows, cols in ((3, 200), (65, 65)):
        M = c.pair.matrix(rows, cols)
        want = np.zeros((rows, cols), dtype=np.uint64)
        for x, y in zip(c.pair.ca.tolist(), c.pair.cb.tolist()):
            want[min(x, rows - 1), min(y, cols - 1)] += 1
        assert np.array_equal(M, want)
    rg = vu.JOINS[2]
    keys, ca, cb = c.pair.joined(0, 7, rg)
    at = c.b.find(*((keys.reshape(-1, 2)[:, 0], keys.reshape(-1, 2)[:, 1]) if k > 32 else (np.zeros(len(keys), dtype=U64), keys)), k)
    assert (at >= 0).all() and np.array_equal(c.b.count[at], cb) and ((cb >= 1) & (cb <= 9)).all() and (ca >= 10 ** 9).all()
    # the profile reads: a sum above 2^32 and a median strictly between min and max exist
    bases, offsets = c.profile_reads()
    counts, valid = vu.window_counts(c.a, bases, offsets, k)
    st = vu.expected_stats(counts, valid, offsets)
    assert (st["sum"] > 2 ** 32).any() and ((st["min"] < st["median"]) & (st["median"] < st["max"])).any()
    assert np.array_equal(counts[offsets[:len(c.a)].astype(np.int64)], c.a.count), "one read a stored k-mer, one window"
    assert (st["windows"][:len(c.a)] == 1).all() and (st["max"][-100:] == 0).all()


def plain_stats(counts, valid, offsets, k, lo, hi):
    out = []
    for i in range(len(offsets) - 1):
        a, b = int(offsets[i]), int(offsets[i + 1])
        w = [int(counts[p]) for p in range(a, b) if p + k <= b and (valid is None or valid[p])]
        w.sort()
        out.append((len(w), sum(lo <= x <= hi for x in w), w[0], w[(len(w) - 1) // 2], w[-1], 0, sum(w)) if w
                   else (0,) * 7)
    return out


@pytest.mark.parametrize("k", [1, 31])
def test_expected_read_statistics_against_a_plain_loop(k):
    counts, valid, offsets = vu.stat_batch(k, seed=k, only=150)
    assert len(offsets) == 151 and offsets[-1] == len(counts) == len(valid)
    for v in (None, valid):
        for lo, hi in vu.STAT_RANGES + [(7, 7)]:
            got = vu.expected_select(counts, v, offsets, k, lo, hi)
            assert [tuple(int(x) for x in row) for row in got.tolist()] == plain_stats(counts, v, offsets, k, lo, hi)
    full = vu.stat_batch(k, seed=k)
    lens = np.diff(full[2].astype(np.int64))
    w = np.maximum(lens - k + 1, 0)
    assert 1900 < len(w) < 2100 and set(w.tolist()) == set(vu.STAT_WINDOWS)
    st = vu.expected_select(*full, k)
    assert int(st["sum"].max()) == 1000 * vu.MAX and (st["windows"] < w).any() and (st["windows"][w > 256] == 0).any()
