"""fk_compare* and the joined bin views (fk_bin_sizes_joined / fk_get_bin_joined) against the CPU oracle,
through the C-ABI only (needs a GPU).  Everything is exact.

Expectations come from two oracle.OracleResults through query_util.OracleTable, never dicts of k-mers:
the two tables' (hi, lo) keys are concatenated, lexsorted and grouped, which gives (ca, cb) for every
k-mer of the union; the matrix is np.add.at over (min(ca, rows - 1), min(cb, cols - 1)); a joined bin is
a boolean mask over one side's bin with the other side's count from the same grouping.

Inputs: `pair_small` (two samples of 3000 reads of one 200 kb genome, half of the reads shared, the
second with 3000 identical reads appended: k-mers on either side only, on both sides with equal and with
different counts, and one side's counts far above the matrix), `pair_heavy` (60 000 reads of a 3 Gb
genome against their first half plus repeats: results with split buckets, staged pieces, counts around
3000 and above 90 000)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import fastkmer_amd as fk
import oracle
from query_util import CONFIGS, OracleTable, pack
from test_gpu_query import REP, heavy_job, small_job
from test_gpu_spectrum import POLY

pytestmark = pytest.mark.gpu

MAX = fk.MAX_COUNT
REC = 114  # fk_synth_record_bytes(100)
SHAPES = [(256, 256), (2, 2), (3, 200), (70, 5)]
JOINS = [(1, MAX, 0, MAX), (1, MAX, 1, MAX), (1, MAX, 0, 0), (2, 3, 1, 1), (1, 1, 256, MAX), (4_000_000_000, MAX, 0, MAX)]


class Pair:
    """Two inputs with the oracle's results over them and (ca, cb) of every k-mer of their union."""

    def __init__(self, fa, fb, k, m, B, tab_a=None, threads=1):
        if tab_a is None:
            ra = oracle.OracleResult(fa, k, m, B, threads=threads)
            tab_a = OracleTable(ra, ra.nbins)
        rb = oracle.OracleResult(fb, k, m, B, threads=threads)
        self._join((fa, fb), k, m, B, rb.nbins, tab_a, OracleTable(rb, rb.nbins))

    @classmethod
    def of_tables(cls, tab_a, tab_b, k, m, B, nbins):
        """A pair over two tables made elsewhere (query_util.OracleTable's fields), without inputs."""
        self = cls.__new__(cls)
        self._join(None, k, m, B, nbins, tab_a, tab_b)
        return self

    def _join(self, fasta, k, m, B, nbins, tab_a, tab_b):
        self.fasta, self.k, self.m, self.B, self.nbins = fasta, k, m, B, nbins
        self.tabs = (tab_a, tab_b)
        na = len(tab_a)
        hi = np.concatenate([t.hi for t in self.tabs])
        lo = np.concatenate([t.lo for t in self.tabs])
        order = np.lexsort((lo, hi))
        sh, sl = hi[order], lo[order]
        new = np.ones(len(order), dtype=np.int64)
        new[1:] = (sh[1:] != sh[:-1]) | (sl[1:] != sl[:-1])
        gid = np.empty(len(order), dtype=np.int64)
        gid[order] = np.cumsum(new) - 1
        nu = int(gid.max()) + 1 if len(gid) else 0
        self.ca, self.cb = np.zeros(nu, dtype=np.int64), np.zeros(nu, dtype=np.int64)
        self.bin = np.zeros(nu, dtype=np.int32)
        self.ca[gid[:na]], self.cb[gid[na:]] = self.tabs[0].count, self.tabs[1].count
        self.bin[gid[:na]], self.bin[gid[na:]] = self.tabs[0].bin, self.tabs[1].bin
        # the other side's count of every k-mer of a side, in that side's table order
        self.other = (self.cb[gid[:na]].astype(np.uint32), self.ca[gid[na:]].astype(np.uint32))

    def matrix(self, rows, cols, mine=None):
        """The joint matrix of side 0 against side 1 over the k-mers selected by `mine` (all)."""
        ca, cb = self.ca, self.cb
        if mine is not None:
            ca, cb = ca[mine], cb[mine]
        M = np.zeros((rows, cols), dtype=np.uint64)
        np.add.at(M, (np.minimum(ca, rows - 1), np.minimum(cb, cols - 1)), 1)
        return M

    def _keep(self, side, rg, at=slice(None)):
        lo, hi, olo, ohi = rg
        c, o = self.tabs[side].count[at], self.other[side][at]
        return (c >= lo) & (c <= hi) & (o >= olo) & (o <= ohi)

    def joined(self, side, b, rg):
        """(keys in fk_get_bin's layout, counts, other counts) of bin b of `side` joined with the other side."""
        t = self.tabs[side]
        at = slice(int(np.searchsorted(t.bin, b, "left")), int(np.searchsorted(t.bin, b, "right")))
        keep = self._keep(side, rg, at)
        return pack(t.hi[at][keep], t.lo[at][keep], self.k), t.count[at][keep], self.other[side][at][keep]

    def sizes(self, side, rg, owner=None, rank=0):
        keep = self._keep(side, rg)
        if owner is not None:
            keep &= owner[self.tabs[side].bin] == rank
        return np.bincount(self.tabs[side].bin[keep], minlength=self.nbins).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def pair_small(k, m, B):
    fa = fk.synth_fasta(3000, 100, 200_000, seed=0xA0 + k)
    fb = fk.synth_fasta(3000, 100, 200_000, seed=0xA0 + k, first_read=1500) + REP
    tab_a = small_job(k, m, B)[1] if (k, m, B) in CONFIGS else None
    p = Pair(fa, fb, k, m, B, tab_a)
    # on the oracle, before any job is trusted: every region of the matrix is populated
    both, only_a, only_b = (p.ca > 0) & (p.cb > 0), p.cb == 0, p.ca == 0
    assert both.sum() > 10_000 and only_a.sum() > 10_000 and only_b.sum() > 10_000
    assert (both & (p.ca != p.cb)).any() and (p.cb > 255).any()
    return p


@functools.lru_cache(maxsize=None)
def pair_heavy(k, m):
    fa, tab_a, _ = heavy_job(k, m)
    assert fa[30_000 * REC - 1:30_000 * REC + 1] == b"\n>"
    return Pair(fa, fa[:30_000 * REC] + POLY + REP, k, m, 16, tab_a, threads=4)


def run_counter(fasta, k, m, B, **kw):
    kc = fk.KmerCounter(k, m, 3, B, **kw)
    kc.ingest(fasta)
    kc.finish()
    return kc


@pytest.fixture(scope="module")
def counted():
    """Counted pairs shared by the tests that only read results: counted(pair) -> (KmerCounter, KmerCounter)."""
    cache = {}

    def get(pair):
        if id(pair) not in cache:
            cache[id(pair)] = tuple(run_counter(f, pair.k, pair.m, pair.B) for f in pair.fasta)
        return cache[id(pair)]

    yield get
    for kcs in cache.values():
        for kc in kcs:
            kc.close()


def check_matrix(ka, kb, pair, rows, cols):
    want = pair.matrix(rows, cols)
    M = ka.compare(kb, rows, cols)
    assert M.dtype == np.uint64 and M.shape == (rows, cols)
    bad = np.argwhere(M != want)
    assert len(bad) == 0, (f"{rows} x {cols}: {len(bad)} entries differ, e.g. {[tuple(x) for x in bad[:4]]}: "
                           f"{[int(M[tuple(x)]) for x in bad[:4]]}, the oracle has {[int(want[tuple(x)]) for x in bad[:4]]}")
    # what needs no oracle
    assert M[0, 0] == 0
    assert np.array_equal(M[1:].sum(axis=1), ka.spectrum(rows)[1:])
    assert np.array_equal(M[:, 1:].sum(axis=0), kb.spectrum(cols)[1:])
    assert np.array_equal(kb.compare(ka, cols, rows), M.T)
    return M


def check_joined_bin(ka, kb, pair, side, b, rg):
    keys, counts, others = ka.get_bin_joined(kb, b, *rg)
    wk, wc, wo = pair.joined(side, b, rg)
    assert np.array_equal(keys, wk), f"bin {b} {rg}: keys / order"
    assert np.array_equal(counts, wc), f"bin {b} {rg}: counts"
    assert np.array_equal(others, wo), f"bin {b} {rg}: counts in the other result"
    assert others.dtype == np.uint32 and counts.dtype == np.uint32
    return len(counts)


def some_bins(pair, side, n=5):
    full = np.nonzero(pair.sizes(side, JOINS[0]))[0]
    return sorted({int(full[i * (len(full) - 1) // (n - 1)]) for i in range(n)})


# 1. the matrix, every configuration
@pytest.mark.parametrize("k,m,B", CONFIGS)
def test_matrix_small(counted, k, m, B):
    pair = pair_small(k, m, B)
    ka, kb = counted(pair)
    for rows, cols in SHAPES:
        M = check_matrix(ka, kb, pair, rows, cols)
        assert int(M.sum()) == len(pair.ca) and M[0, 1:].any() and M[1:, 0].any() and M[1:, 1:].any()
    assert check_matrix(ka, kb, pair, 256, 256)[:, 255].sum() > 0  # the repeats, clamped into the last column


# ... through the kernel of results of 2^32 k-mers and more (64-bit tile entries; a test hook)
def test_matrix_small_wide_tile(monkeypatch):
    monkeypatch.setenv("FASTKMER_DEBUG_SPECTRUM_WIDE", "1")
    pair = pair_small(28, 10, 2048)
    with run_counter(pair.fasta[0], 28, 10, 2048) as ka, run_counter(pair.fasta[1], 28, 10, 2048) as kb:
        for rows, cols in SHAPES:
            check_matrix(ka, kb, pair, rows, cols)


# 2. results with different cell bits: A's cell index means nothing in B
@pytest.mark.parametrize("k,m,B", [(21, 7, 64), (55, 12, 64)])
def test_different_cell_bits(monkeypatch, k, m, B):
    pair = pair_small(k, m, B)
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2")  # cells of two keys: buckets of many cells
    ka = run_counter(pair.fasta[0], k, m, B)
    monkeypatch.delenv("FASTKMER_DEBUG_CELL_TARGET")
    kb = run_counter(pair.fasta[1], k, m, B)
    try:
        sa, sb = ka.stats(), kb.stats()
        assert 4 * sa["buckets"] < (ka.num_bins << sa["fine_bits"]), sa
        assert sa["fine_bits"] != sb["fine_bits"], (sa["fine_bits"], sb["fine_bits"])
        for rows, cols in SHAPES:
            check_matrix(ka, kb, pair, rows, cols)
        for side, (x, y) in enumerate(((ka, kb), (kb, ka))):
            for rg in JOINS[:4]:
                want = pair.sizes(side, rg)
                assert np.array_equal(x.bin_sizes_joined(y, *rg), want), (side, rg)
                for b in some_bins(pair, side):
                    assert check_joined_bin(x, y, pair, side, b, rg) == want[b]
    finally:
        ka.close()
        kb.close()


# 3. a result against itself
@pytest.mark.parametrize("k,m,B", [CONFIGS[0], CONFIGS[3]])
def test_self_comparison_is_the_spectrum(counted, k, m, B):
    pair = pair_small(k, m, B)
    for kc in counted(pair):
        for n in (2, 8, 64, 300):
            M = kc.compare(kc, n, n)
            assert np.array_equal(np.diag(M), kc.spectrum(n)) and int(M.sum()) == int(np.trace(M)) > 0
    kb = counted(pair)[1]
    assert kb.compare(kb, 300, 300)[299, 299] > 0  # the repeats


# 4. split buckets and staged pieces
def check_heavy(ka, kb, pair):
    for kc in (ka, kb):
        assert kc.stats()["split_buckets"] > 100, kc.stats()
    M = check_matrix(ka, kb, pair, 4096, 4096)  # ... and transposed: the tail is a column, then a row
    assert M[3000, 3000] > 0 and M[0, 4095] > 0  # the repeats of both samples and the poly-A k-mer: global atomics
    for side, (x, y) in enumerate(((ka, kb), (kb, ka))):
        for rg in ((1, MAX, 1, MAX), (2, MAX, 0, MAX)):
            want = pair.sizes(side, rg)
            assert np.array_equal(x.bin_sizes_joined(y, *rg), want)
            for b in (0, 7, 15):
                assert check_joined_bin(x, y, pair, side, b, rg) == want[b] > 0


@pytest.mark.parametrize("k,m", [(28, 10), (55, 12)])
def test_heavy_split_buckets(monkeypatch, k, m):
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2600")
    pair = pair_heavy(k, m)
    assert (pair.cb >= 3000).any() and (pair.cb > 90_000).any() and (pair.ca >= 3000).any()
    with run_counter(pair.fasta[0], k, m, 16) as ka, run_counter(pair.fasta[1], k, m, 16) as kb:
        check_heavy(ka, kb, pair)


def test_heavy_staged_pieces(monkeypatch):
    import torch
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2600")
    pair = pair_heavy(28, 10)
    with run_counter(pair.fasta[1], 28, 10, 16) as kb:
        monkeypatch.setenv("FASTKMER_INGEST_SEG", str(262144))
        monkeypatch.setenv("FASTKMER_PIECE_BYTES", str(524288))
        host = torch.frombuffer(bytearray(pair.fasta[0]), dtype=torch.uint8).pin_memory()
        with fk.KmerCounter(28, 10, 3, 16) as ka:
            ka.ingest_ptr(host.data_ptr(), host.numel())
            ka.finish()
            assert ka.stats()["pieces_counted"] == 4, ka.stats()
            check_heavy(ka, kb, pair)


# 5. joined views
@pytest.mark.parametrize("k,m,B", [CONFIGS[0], CONFIGS[3]])
def test_joined_views_small(counted, k, m, B):
    pair = pair_small(k, m, B)
    ka, kb = counted(pair)
    kw = 2 if k > 32 else 1
    kept_any = 0
    for i, rg in enumerate(JOINS):
        want = pair.sizes(0, rg)
        got = ka.bin_sizes_joined(kb, *rg)
        assert np.array_equal(got, want), f"{rg}: bins {np.nonzero(got != want)[0][:5]} differ"
        kept_any += int(want.any())
        bins = np.nonzero(pair.sizes(0, JOINS[0]))[0].tolist() if i < 2 else some_bins(pair, 0)
        for b in bins:
            assert check_joined_bin(ka, kb, pair, 0, b, rg) == want[b]
    assert kept_any >= 4 and not pair.sizes(0, JOINS[5]).any()  # the ranges are not all empty on this input
    # the other direction, and a range only the repeats of the second sample meet
    for rg in JOINS + [(256, MAX, 0, 0)]:
        assert np.array_equal(kb.bin_sizes_joined(ka, *rg), pair.sizes(1, rg)), rg
    rep = (256, MAX, 0, 0)
    assert pair.sizes(1, rep).sum() > 0
    for b in np.nonzero(pair.sizes(1, rep))[0][:3].tolist():
        assert check_joined_bin(kb, ka, pair, 1, b, rep) > 0
    parts = [0, 0]
    for b in some_bins(pair, 0):
        ukeys, ucounts = ka.get_bin(b)
        keys, counts, others = ka.get_bin_joined(kb, b)  # (1, MAX, 0, MAX)
        assert np.array_equal(keys, ukeys) and np.array_equal(counts, ucounts)
        assert np.array_equal(others, kb.query(ukeys))
        # intersection and difference partition the bin
        ik, ic, io = ka.intersect_bin(kb, b)
        sk, sc, so = ka.subtract_bin(kb, b)
        assert (io > 0).all() and not so.any() and len(ic) + len(sc) == len(ucounts)
        parts[0] += len(ic)
        parts[1] += len(sc)
        merged = np.concatenate([ik.reshape(-1, kw), sk.reshape(-1, kw)])
        order = np.lexsort((merged[:, -1], merged[:, 0]))
        assert np.array_equal(merged[order].reshape(-1), ukeys)
        assert np.array_equal(np.concatenate([ic, sc])[order], ucounts)
        assert np.array_equal(np.concatenate([io, so])[order], others)
    assert parts[0] > 0 and parts[1] > 0  # neither side of the partition is empty on these bins


# 6. the buffer rules (fk_get_bin_range's)
def test_joined_buffer_rules(counted):
    pair = pair_small(28, 10, 2048)
    ka, kb = counted(pair)
    L, rg = fk.lib(), (1, MAX, 1, MAX)
    want = pair.sizes(0, rg)
    b = int(np.argmax(want))
    want_n = int(want[b])
    assert want_n > 1
    full = pair.joined(0, b, rg)
    keys, counts, others = np.zeros(want_n, dtype=np.uint64), np.full(want_n, 77, dtype=np.uint32), np.full(want_n, 78, dtype=np.uint32)
    n = ctypes.c_size_t(0)

    def call(kp, cp, op, cap, bin_=b):
        n.value = 0
        return L.fk_get_bin_joined(ka._h, kb._h, bin_, *rg, kp, cp, op, cap, ctypes.byref(n))

    assert call(keys.ctypes.data, counts.ctypes.data, others.ctypes.data, want_n - 1) == -6
    assert n.value == want_n and not keys.any() and (counts == 77).all() and (others == 78).all()
    assert call(None, None, None, want_n) == 0 and n.value == want_n
    assert call(None, None, None, 0) == -6 and n.value == want_n
    assert call(keys.ctypes.data, None, None, want_n) == 0 and n.value == want_n and np.array_equal(keys, full[0])
    assert (counts == 77).all() and (others == 78).all()
    assert call(None, counts.ctypes.data, None, want_n) == 0 and np.array_equal(counts, full[1]) and (others == 78).all()
    assert call(None, None, others.ctypes.data, want_n) == 0 and np.array_equal(others, full[2])
    for bad in (-1, pair.nbins):
        assert call(None, None, None, 0, bad) == -6
    assert L.fk_get_bin_joined(ka._h, kb._h, b, *rg, None, None, None, 0, None) == -1


# 7. states, arguments, empty jobs
def _raw_calls(ka, kb, rows=8, cols=8, rg=(1, MAX, 0, MAX)):
    """The four C calls' return codes."""
    import torch
    L = fk.lib()
    mat = np.zeros(max(rows * cols, 1), dtype=np.uint64)
    d_mat = torch.zeros(max(min(rows * cols, 1 << 24), 1), dtype=torch.int64, device="cuda")
    sizes = np.zeros(ka.num_bins, dtype=np.uint64)
    cnt = ctypes.c_size_t(0)
    rcs = [L.fk_compare(ka._h, kb._h, mat.ctypes.data if rows * cols <= 1 << 24 else None, rows, cols),
           L.fk_compare_device(ka._h, kb._h, ctypes.c_void_p(d_mat.data_ptr()), rows, cols),
           L.fk_bin_sizes_joined(ka._h, kb._h, *rg, sizes.ctypes.data),
           L.fk_get_bin_joined(ka._h, kb._h, 0, *rg, None, None, None, 1 << 40, ctypes.byref(cnt))]
    torch.cuda.synchronize()
    return rcs


def test_states_arguments_and_empty_jobs(counted):
    k, m, B = 28, 10, 2048
    pair = pair_small(k, m, B)
    ka, kb = counted(pair)
    with fk.KmerCounter(k, m, 3, B) as kc:
        assert _raw_calls(kc, kb) == [-2] * 4 and _raw_calls(ka, kc) == [-2] * 4  # FK_E_STATE: nothing counted
        kc.ingest(pair.fasta[0])
        assert _raw_calls(kc, kb) == [-2] * 4 and _raw_calls(ka, kc) == [-2] * 4
        kc.finish()
        assert _raw_calls(kc, kb) == [0] * 4 and _raw_calls(ka, kc) == [0] * 4
        assert np.array_equal(kc.compare(kb, 8, 8), pair.matrix(8, 8))
        assert np.array_equal(kc.compare(ka, 8, 8), ka.compare(ka, 8, 8))
    # FK_E_INVALID: configurations that do not count the same k-mers into the same bins
    for kw in (dict(use_ht=True), dict(k=27), dict(m=9), dict(B=1024), dict(x=2)):
        cfg = dict(dict(k=k, m=m, x=3, B=B), **kw)
        with fk.KmerCounter(cfg["k"], cfg["m"], cfg["x"], cfg["B"], use_ht=cfg.get("use_ht", False)) as kc:
            kc.ingest(pair.fasta[1])
            kc.finish()
            want = [0] * 4 if "x" in kw else [-1] * 4  # x may differ
            assert _raw_calls(ka, kc) == want and _raw_calls(kc, ka) == want, kw
            if "x" not in kw:
                assert list(kw)[0].replace("B", "bin count") in fk.lib().fk_last_error().decode(), kw
            else:
                assert np.array_equal(ka.compare(kc, 8, 8), pair.matrix(8, 8))
    with fk.KmerCounter(k, m, 3, B, n_ranks=2, rank=0) as kc:
        assert _raw_calls(ka, kc) == [-1] * 4 and b"n_ranks" in fk.lib().fk_last_error()
    # bad shapes (the matrix calls) and bad ranges (the joined calls)
    for rows, cols in ((1, 8), (8, 1), (0, 0), (4096, 4097), (65537, 2), (2, 65537)):
        assert _raw_calls(ka, kb, rows, cols)[:2] == [-1, -1], (rows, cols)
    assert _raw_calls(ka, kb, 65536, 256)[:2] == [0, 0] and _raw_calls(ka, kb, 2, 65536)[:2] == [0, 0]
    assert _raw_calls(ka, kb, rg=(0, MAX, 0, MAX))[2:] == [-1, -1]
    assert _raw_calls(ka, kb, rg=(3, 2, 0, MAX))[2:] == [-1, -1]
    assert _raw_calls(ka, kb, rg=(1, MAX, 2, 1))[2:] == [-1, -1]
    L = fk.lib()
    assert L.fk_compare(ka._h, kb._h, None, 8, 8) == -1 and L.fk_compare_device(ka._h, kb._h, None, 8, 8) == -1
    assert L.fk_bin_sizes_joined(ka._h, kb._h, 1, MAX, 0, MAX, None) == -1
    for call in (lambda: ka.compare(kb, 1, 8), lambda: ka.bin_sizes_joined(kb, min_count=0),
                 lambda: ka.get_bin_joined(kb, 0, other_min=2, other_max=1)):
        with pytest.raises(fk.FastKmerError) as e:
            call()
        assert e.value.code == -1
    # an empty job on either side: zeros, or only row 0 / column 0
    with run_counter(b"", k, m, B) as empty:
        M = ka.compare(empty, 8, 8)
        assert np.array_equal(M[:, 0], ka.spectrum(8)) and not M[:, 1:].any()
        M = empty.compare(ka, 8, 8)
        assert np.array_equal(M[0], ka.spectrum(8)) and not M[1:].any()
        assert not empty.compare(empty, 8, 8).any()
        assert _raw_calls(empty, ka) == [0] * 4 and _raw_calls(ka, empty) == [0] * 4
        assert not empty.bin_sizes_joined(ka).any() and len(empty.get_bin_joined(ka, 0)[1]) == 0
        assert np.array_equal(ka.bin_sizes_joined(empty), ka.bin_sizes()) and not ka.bin_sizes_joined(empty, other_min=1).any()
        b = int(np.argmax(ka.bin_sizes()))
        keys, counts, others = ka.subtract_bin(empty, b)
        assert np.array_equal(keys, ka.get_bin(b)[0]) and np.array_equal(counts, ka.get_bin(b)[1]) and not others.any()


# 8. the calls only read
def test_the_new_calls_only_read_both_results(tmp_path):
    pair = pair_small(28, 10, 2048)
    with run_counter(pair.fasta[0], 28, 10, 2048) as ka, run_counter(pair.fasta[1], 28, 10, 2048) as kb:
        some = np.nonzero(pair.sizes(0, (1, MAX, 1, MAX)))[0][[0, 7, -1]].tolist()
        keys = [pack(t.hi[:1000], t.lo[:1000], 28) for t in pair.tabs]

        def readers():
            out = []
            for kc in (ka, kb):
                out += [a for b in some for a in kc.get_bin(b)]
                out += [np.frombuffer(kc.bin_text(some[0]).encode(), dtype=np.uint8)]
                out += [kc.query(keys[0]), kc.query(keys[1]), kc.spectrum(64)]
            return out

        before = readers()
        M = ka.compare(kb, 64, 64)
        for b in some:
            ka.get_bin_joined(kb, b, other_min=1)
        ka.bin_sizes_joined(kb, 2, None, 0, 0)
        after = readers()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        assert np.array_equal(ka.compare(kb, 64, 64), M) and np.array_equal(M, pair.matrix(64, 64))  # overwritten
        kb.compare(ka, 64, 64), kb.get_bin_joined(ka, some[0])
        after = readers()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        ka.write_bins(str(tmp_path / "a"))  # materialises the dense copy; the comparison still walks the buckets
        assert np.array_equal(ka.compare(kb, 64, 64), M)
        check_joined_bin(ka, kb, pair, 0, some[1], (1, MAX, 1, MAX))


# 9. the device form on the caller's stream
def test_compare_ptr_on_the_callers_stream():
    import torch
    pair = pair_small(28, 10, 2048)
    with run_counter(pair.fasta[1], 28, 10, 2048) as kb:  # on its own stream throughout
        for stream in (None, torch.cuda.Stream()):  # torch's default stream, then a side stream
            with run_counter(pair.fasta[0], 28, 10, 2048) as ka:  # closed before the stream goes away
                with torch.cuda.stream(stream):
                    ka.set_stream(torch.cuda.current_stream().cuda_stream)
                    for rows, cols in ((2, 2), (70, 300)):
                        want = pair.matrix(rows, cols)
                        assert np.array_equal(ka.compare(kb, rows, cols), want)
                        d = torch.full((rows * cols,), -7, dtype=torch.int64, device="cuda")
                        d_self = torch.full((rows * cols,), 1 << 40, dtype=torch.int64, device="cuda")
                        for _ in range(2):  # overwritten, not accumulated into
                            ka.compare_ptr(kb, d.data_ptr(), rows, cols)
                            ka.compare_ptr(ka, d_self.data_ptr(), rows, cols)
                        torch.cuda.current_stream().synchronize()
                        assert np.array_equal(d.cpu().numpy().view(np.uint64).reshape(rows, cols), want)
                        assert np.array_equal(d_self.cpu().numpy().view(np.uint64).reshape(rows, cols), ka.compare(ka, rows, cols))


# 10. ranks: a rank's matrix covers the bins it owns; the ranks' sum is the job's
def check_ranks(ranks_a, ranks_b, pair, owner):
    total = np.zeros((300, 70), dtype=np.uint64)
    rg = (1, MAX, 1, MAX)
    sizes = np.zeros(pair.nbins, dtype=np.uint64)
    for r, (ka, kb) in enumerate(zip(ranks_a, ranks_b)):
        mine = owner[pair.bin] == r
        assert mine.any() and not mine.all()
        M = ka.compare(kb, 300, 70)
        assert np.array_equal(M, pair.matrix(300, 70, mine=mine)), f"rank {r}"
        assert np.array_equal(kb.compare(ka, 70, 300), M.T)
        total += M
        s = ka.bin_sizes_joined(kb, *rg)
        assert s.any() and not s[owner != r].any(), f"rank {r} reports sizes for bins it does not own"
        assert np.array_equal(s, pair.sizes(0, rg, owner, r))
        sizes += s
        own = int(np.nonzero((owner == r) & (s > 0))[0][0])
        check_joined_bin(ka, kb, pair, 0, own, rg)
        other = int(np.nonzero((owner != r) & (pair.sizes(0, rg) > 0))[0][0])
        assert len(ka.get_bin_joined(kb, other, *rg)[1]) == 0
    assert np.array_equal(total, pair.matrix(300, 70)) and np.array_equal(sizes, pair.sizes(0, rg))


def test_ranks_two_exchanging():
    from test_gpu_comm import record_shards, run_local_job
    pair = pair_small(28, 10, 2048)
    groups = [run_local_job(record_shards(f, 2), 28, 10, 3, 2048) for f in pair.fasta]
    try:
        owner = groups[0][0].bin_owners()
        assert np.array_equal(owner, np.arange(2048) % 2)
        check_ranks(groups[0], groups[1], pair, owner)
        with pytest.raises(fk.FastKmerError) as e:  # a rank against another rank's result
            groups[0][0].compare(groups[1][1], 8, 8)
        assert e.value.code == -1 and "rank" in str(e.value)
    finally:
        for kc in groups[0] + groups[1]:
            kc.close()


def _exchange_by_hand(ranks, shards, owner=None):
    """map -> (owners) -> emit -> reduce over in-process ranks without a communicator; returns the owners."""
    import torch
    G = len(ranks)
    sizes = np.zeros(ranks[0].num_bins, dtype=np.uint64)
    for r in range(G):
        ranks[r].ingest(shards[r])
        ranks[r].map()
        sizes += ranks[r].map_bin_kmers()
    if owner is None:
        owner = fk.lpt_owners(sizes, G)
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
    return np.asarray(owner)


def test_ranks_three_with_lpt_owners():
    k, m, B, G = 28, 10, 2048, 3
    pair = pair_small(k, m, B)
    groups = [[fk.KmerCounter(k, m, 3, B, n_ranks=G, rank=r) for r in range(G)] for _ in range(2)]
    try:
        cut = lambda f: [f[r * REC * (len(f) // REC // G):(r + 1) * REC * (len(f) // REC // G) if r < G - 1 else len(f)]
                         for r in range(G)]
        owner = _exchange_by_hand(groups[0], cut(pair.fasta[0]))
        assert not np.array_equal(owner, np.arange(B) % G)
        _exchange_by_hand(groups[1], cut(pair.fasta[1]), owner)  # the same owner table on both samples
        check_ranks(groups[0], groups[1], pair, owner)
        # contexts with different owner tables are refused
        with fk.KmerCounter(k, m, 3, B, n_ranks=G, rank=0) as plain:
            assert _raw_calls(groups[0][0], plain) == [-1] * 4 and b"owners" in fk.lib().fk_last_error()
            assert _raw_calls(plain, groups[0][0]) == [-1] * 4
    finally:
        for kc in groups[0] + groups[1]:
            kc.close()


# 11. the CLI
def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))} if os.path.isdir(d) else {}


def test_cli_compare(tmp_path):
    pair = pair_small(28, 10, 2048)
    paths = [tmp_path / "a.fa", tmp_path / "b.fa"]
    for p, f in zip(paths, pair.fasta):
        p.write_bytes(f)
    base = {k: v for k, v in os.environ.items() if not k.startswith("FASTKMER_CLI_")}

    def run(prefix, write, **env):
        r = subprocess.run([fk.CLI_PATH, "28", "10", "3", "2048", "0", "0", str(paths[0]), str(tmp_path) + "/", prefix,
                            str(write), "0", "0"], capture_output=True, text=True, env=dict(base, **env))
        assert r.returncode == 0, r.stderr
        return _files(tmp_path / f"{prefix}k28_m10_x3_b2048_s0"), r.stdout

    def tsv(n):
        M = pair.matrix(n, n)
        return "".join(f"{a}\t{b}\t{int(M[a, b])}\n" for a in range(n) for b in range(n) if M[a, b]).encode()

    plain, out = run("plain_", 1)  # without the variable: as before
    assert "compare.tsv" not in plain and "Comparison" not in out and len(plain) > 2000
    got, out = run("cmp_", 1, FASTKMER_CLI_COMPARE=str(paths[1]))
    assert got.pop("compare.tsv") == tsv(256) and got == plain and "Comparison" in out  # the bin files byte for byte
    got, _ = run("n_", 0, FASTKMER_CLI_COMPARE=str(paths[1]), FASTKMER_CLI_COMPARE_N="5")  # write = 0: the matrix only
    assert got == {"compare.tsv": tsv(5)} and got["compare.tsv"].splitlines()[0].startswith(b"0\t1\t")
    r = subprocess.run([fk.CLI_PATH, "28", "10", "3", "2048", "0", "0", str(paths[0]), str(tmp_path) + "/", "bad_", "0", "0", "0"],
                       capture_output=True, env=dict(base, FASTKMER_CLI_COMPARE=str(tmp_path / "missing.fa")))
    assert r.returncode == 1 and b"cannot open" in r.stderr and b"missing.fa" in r.stderr
