"""The model behind test_gpu_every_k.py, test_gpu_view_counts.py and test_gpu_read_stats_select.py: the
inputs, the chosen counts and every expectation, in numpy and plain Python over oracle.OracleResult.
Nothing here calls the library's result views; test_views_util.py checks the model without a GPU.

Part 1 (every k): one small FASTA per k whose reads cover every class of input (random, repeated,
reads holding N / lower case / '\\r', poly-A and poly-T, a self-complementary repeat, reads of exactly k,
k - 1 and 0 bases) and a second one sharing half of them, counted by the oracle under (k, m(k), B(k)).

Part 2 (chosen counts): about 6000 canonical k-mers binned by the oracle, with counts dealt from a
palette that holds every digit width, the edges of the LDS tables and the top of the 32-bit range, as two
results A and B in which all 37 x 37 pairs of counts occur.

Part 3 (read statistics): position-indexed count / valid / offset arrays and their statistics by np.sort."""
import functools

import numpy as np

import oracle
from query_util import OracleTable, U64, canonical, is_kmer, pack, revcomp
from test_gpu_compare import Pair
from test_gpu_reads import csr, expected_stats, revcomp_read, windows
from test_gpu_spectrum import Job

MAX = 0xFFFFFFFF
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- keys, strings and tables
def key_bases(hi, lo, k):
    """The k bases of every key as a uint8 matrix [n, k], first base first."""
    out = np.empty((len(lo), k), dtype=np.uint8)
    for j in range(k):
        p = k - 1 - j  # base j sits in bits [2p, 2p + 2)
        w = lo if p < 32 else hi
        out[:, j] = ACGT[((w >> U64(2 * (p % 32))) & U64(3)).astype(np.int64)]
    return out


def keys_fasta(hi, lo, k):
    """A FASTA with one k-base read per key."""
    rows = np.empty((len(lo), k + 4), dtype=np.uint8)
    rows[:, :3] = np.frombuffer(b">k\n", dtype=np.uint8)
    rows[:, 3:k + 3] = key_bases(hi, lo, k)
    rows[:, k + 3] = ord("\n")
    return rows.tobytes()


def random_keys(rng, k, n):
    """n uniform 2k-bit keys as (hi, lo)."""
    hi, lo = rng.integers(0, 2 ** 64, size=(2, n), dtype=U64)
    if k < 32:
        lo &= U64((1 << (2 * k)) - 1)
    if k <= 32:
        hi[:] = 0
    elif k < 64:
        hi &= U64((1 << (2 * k - 64)) - 1)
    return hi, lo


class Table(OracleTable):
    """An OracleTable over arrays the caller chose: hi, lo, count, bin in (bin, key) order."""

    def __init__(self, hi, lo, count, bin_):
        self.hi, self.lo = np.ascontiguousarray(hi, dtype=U64), np.ascontiguousarray(lo, dtype=U64)
        self.count, self.bin = np.ascontiguousarray(count, dtype=np.uint32), np.ascontiguousarray(bin_, dtype=np.int32)
        cut = np.nonzero(np.diff(self.bin))[0] + 1 if len(self.bin) else np.zeros(0, dtype=np.int64)
        self.first = np.concatenate([[0], cut]).tolist() if len(self.bin) else []
        self.last = np.concatenate([cut - 1, [len(self.bin) - 1]]).tolist() if len(self.bin) else []


def oracle_bins(hi, lo, k, m, B):
    """The oracle's bin of every key (either strand): the keys joined by N are one read whose super-k-mers are the
    keys one by one, and oracle.trace_read names the bin of each."""
    n = len(lo)
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    rows = np.full((n, k + 1), ord("N"), dtype=np.uint8)
    rows[:, :k] = key_bases(hi, lo, k)
    trace = np.array(oracle.trace_read(rows.tobytes(), k, m, B), dtype=np.int64).reshape(-1, 3)
    assert len(trace) == n and np.array_equal(trace[:, 0], np.arange(n) * (k + 1)) and (trace[:, 1] == k).all()
    return trace[:, 2].astype(np.int32)


def key_lines(hi, lo, count, k):
    """'kmer<TAB>count<LF>' of every (key, count) as a list of bytes."""
    names = key_bases(hi, lo, k)
    return [r.tobytes() + b"\t%d\n" % c for r, c in zip(names, count.tolist())]


def counted_table(reads, k, m, B):
    """The result of counting reads, without a second run of the oracle's counter: the canonical keys of the valid
    windows (test_gpu_reads.windows) counted by np.unique, binned by oracle_bins, in (bin, key) order.
    test_views_util.py holds it against oracle.OracleResult for every k."""
    bases, offsets = csr(reads)
    _, hi, lo = windows(bases, offsets, k)
    chi, clo = canonical(hi, lo, k)
    order = np.lexsort((clo, chi))
    sh, sl = chi[order], clo[order]
    new = np.ones(len(order), dtype=bool)
    new[1:] = (sh[1:] != sh[:-1]) | (sl[1:] != sl[:-1])
    first = np.nonzero(new)[0]
    uh, ul, count = sh[first], sl[first], np.diff(np.concatenate([first, [len(order)]]))
    bins = oracle_bins(uh, ul, k, m, B)
    by_bin = np.argsort(bins, kind="stable")
    return Table(uh[by_bin], ul[by_bin], count[by_bin], bins[by_bin])


def table_texts(tab, k, lo=1, hi=MAX, eof=True):
    """{'bin<b>': bytes} of a table filtered to lo <= count <= hi: a bin with no kept line has no file."""
    lines = key_lines(tab.hi, tab.lo, tab.count, k)
    keep = ((tab.count >= lo) & (tab.count <= hi)).tolist()
    out = {}
    for a, b in zip(tab.first, tab.last):
        kept = [ln for ln, ok in zip(lines[a:b + 1], keep[a:b + 1]) if ok]
        if kept:
            out[f"bin{int(tab.bin[a])}"] = b"".join(kept) + (b"EOF" if eof else b"")
    return out


def spectrum(count, n):
    """(hist, tail k-mers): hist = bincount(min(count, n - 1)), tail = the Python-int sum of the counts >= n - 1."""
    c = np.asarray(count).astype(np.int64)
    return np.bincount(np.minimum(c, n - 1), minlength=n).astype(np.uint64), sum(int(x) for x in c[c >= n - 1])


def range_sizes(tab, nbins, lo, hi):
    keep = (tab.count >= lo) & (tab.count <= hi)
    return np.bincount(tab.bin[keep], minlength=nbins).astype(np.uint64)


def range_bin(tab, k, b, lo, hi):
    """(keys in fk_get_bin's layout, counts) of bin b filtered to lo <= count <= hi, both inclusive."""
    at = slice(int(np.searchsorted(tab.bin, b, "left")), int(np.searchsorted(tab.bin, b, "right")))
    keep = (tab.count[at] >= lo) & (tab.count[at] <= hi)
    return pack(tab.hi[at][keep], tab.lo[at][keep], k), tab.count[at][keep]


def window_counts(tab, bases, offsets, k):
    """(counts, valid) by base position: test_gpu_reads.windows plus a table lookup."""
    valid, hi, lo = windows(bases, offsets, k)
    counts = np.zeros(len(bases), dtype=np.uint32)
    counts[valid] = tab.expected(hi, lo, k)
    return counts, valid.astype(np.uint8)


# ---- part 1: every k
def m_of(k):
    return min(k, 1 + (7 * k) % 15)


def B_of(k):
    return (1, 64, 2048)[k % 3]


def _rand_read(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


@functools.lru_cache(maxsize=None)
def _shared_reads():
    """The reads every k shares, by class."""
    rng = np.random.default_rng(0x51EE7)
    rand = [_rand_read(rng, int(rng.integers(0, 151))) for _ in range(300)]
    long_ones = [i for i, r in enumerate(rand) if len(r) >= 70]
    repeated = [rand[i] for i in long_ones[:20]]
    noisy = []
    for ch in (b"N", b"g", b"\r"):  # a byte that is no base at position 70 of 150: 70 bases before, 79 after
        r = bytearray(_rand_read(rng, 150))
        r[70:71] = ch
        noisy.append(bytes(r))
    new = [_rand_read(rng, int(rng.integers(0, 151))) for _ in range(150)]
    return {"random": rand, "repeated": repeated, "noisy": noisy, "polyA": b"A" * 200, "polyT": b"T" * 200,
            "acgt": b"ACGT" * 50, "new": new}


def to_fasta(reads):
    return b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads))


class EveryK:
    """The two inputs of one k with the oracle's results: job (first input), pair (first against second)."""

    def __init__(self, k):
        self.k, self.m, self.B = k, m_of(k), B_of(k)
        s = _shared_reads()
        rng = np.random.default_rng(1000 + k)
        self.exact, self.short = _rand_read(rng, k), _rand_read(rng, k - 1)
        self.reads = (s["random"] + s["repeated"] * 2 + s["noisy"] + [s["polyA"], s["polyT"], s["acgt"]]
                      + [self.exact, self.short, b""])
        self.reads2 = self.reads[:len(self.reads) // 2] + s["new"] + [s["polyA"]]
        self.fasta, self.fasta2 = to_fasta(self.reads), to_fasta(self.reads2)
        self.job = Job(self.fasta, k, self.m, self.B)
        self.tab, self.ref, self.nbins = self.job.tab, self.job.ref, self.job.nbins
        self.top = int(self.tab.count.max())
        self.check_classes()
        self.tab2 = counted_table(self.reads2, k, self.m, self.B)
        self.pair = Pair.of_tables(self.tab, self.tab2, k, self.m, self.B, self.nbins)

    def counts_of(self, reads):
        """The oracle's count of every valid window of reads, and how many windows exist."""
        bases, offsets = csr(reads)
        counts, valid = window_counts(self.tab, bases, offsets, self.k)
        exist = sum(max(len(r) - self.k + 1, 0) for r in reads)
        return counts[valid != 0], exist

    def check_classes(self):
        """On the oracle's result: every class of read put at least one k-mer into it (every k <= 64 allows it)."""
        k, s = self.k, _shared_reads()
        assert 20_000 < len(self.fasta) < 32_000 and len(self.reads) == 349
        c, n = self.counts_of([r for r in s["random"][200:] if len(r) >= k])
        assert len(c) == n > 0 and c.min() >= 1
        c, n = self.counts_of([r for r in s["repeated"] if len(r) >= k])
        assert len(c) == n > 0 and c.min() >= 3, "a read given three times counts three times"
        for r in s["noisy"]:
            c, n = self.counts_of([r])
            assert 0 < len(c) == n - k and c.min() >= 1, "the bad byte removes k windows and leaves some on either side"
        at = self.tab.find(np.zeros(1, dtype=U64), np.zeros(1, dtype=U64), k)
        assert at[0] >= 0 and self.tab.count[at[0]] >= 2 * (201 - k), "poly-A and poly-T share canonical key 0"
        b, o = csr([s["acgt"]])
        _, hi, lo = windows(b, o, k)
        rh, rl = revcomp(hi, lo, k)
        own = (rh == hi) & (rl == lo)  # at even k the windows at two of the four phases are their own reverse complements
        assert len(lo) == 201 - k and own.sum() == (0 if k % 2 else sum(1 for p in range(201 - k) if (p + k // 2) % 2 == 0))
        c, n = self.counts_of([s["acgt"]])
        assert len(c) == n and c.min() >= (201 - k) // 4
        c, n = self.counts_of([self.exact, self.short, b""])
        assert len(c) == n == 1 and c[0] >= 1
        assert self.ref.total_kmers == int(self.tab.count.sum(dtype=np.uint64)) and self.ref.distinct == len(self.tab)

    def profile_reads(self):
        """The reads appended to reads_csr(input): a reverse complement, 50 random reads, more than one tile joined."""
        rng = np.random.default_rng(2000 + self.k)
        clean = next(r for r in self.reads if len(r) >= 100 and set(r) <= set(b"ACGT"))
        joined = b"".join(self.reads[:100])
        assert len(joined) > 4096 + 64
        return [revcomp_read(clean)] + [_rand_read(rng, int(rng.integers(0, 151))) for _ in range(50)] + [joined]

    def probes(self):
        """(hi, lo, want count, want bin) of the lookups: every stored key on both strands, every stored key +- 1,
        2000 random keys, and for k < 64 keys with one bit above 2k - 1, which are no k-mers: (0, -1)."""
        from query_util import add
        k, t = self.k, self.tab
        rng = np.random.default_rng(3000 + k)
        rh, rl = revcomp(t.hi, t.lo, k)
        up, down, rnd = add(t.hi, t.lo, 1), add(t.hi, t.lo, -1), random_keys(rng, k, 2000)
        hi = np.concatenate([t.hi, rh, up[0], down[0], rnd[0]])
        lo = np.concatenate([t.lo, rl, up[1], down[1], rnd[1]])
        if k < 64 and k != 32:  # one bit above 2k - 1 set in stored keys (a one-word key has no bit 64 to set)
            bits = np.arange(2 * k, 64 if k < 32 else 128)
            bh = np.where(bits >= 64, U64(1) << (bits % 64).astype(U64), U64(0)).astype(U64)
            bl = np.where(bits < 64, U64(1) << (bits % 64).astype(U64), U64(0)).astype(U64)
            src = rng.integers(0, len(t), len(bits))
            hi, lo = np.concatenate([hi, t.hi[src] | bh]), np.concatenate([lo, t.lo[src] | bl])
        if k <= 32:
            hi[:] = 0  # a one-word key has no high word: +- 1 wraps inside 64 bits
        ok = is_kmer(hi, lo, k)
        assert (~ok).sum() >= (0 if k in (32, 64) else (64 if k < 32 else 128) - 2 * k)
        at = t.find(hi[ok], lo[ok], k)
        count, bin_ = np.zeros(len(lo), dtype=np.uint32), np.full(len(lo), -1, dtype=np.int32)
        count[ok] = np.where(at >= 0, t.count[np.maximum(at, 0)], 0)
        bin_[ok] = oracle_bins(hi[ok], lo[ok], k, self.m, self.B)
        assert np.array_equal(bin_[:len(t)], t.bin) and np.array_equal(bin_[len(t):2 * len(t)], t.bin)
        return hi, lo, count, bin_


@functools.lru_cache(maxsize=2)
def every_k(k):
    return EveryK(k)


# ---- part 2: results with chosen counts
PALETTE = [1, 2, 3, 9, 10, 62, 63, 64, 65, 99, 100, 254, 255, 256, 999, 1000, 1023, 1024, 1025, 9999, 10 ** 4, 65535,
           65536, 10 ** 5 - 1, 10 ** 5, 10 ** 6 - 1, 10 ** 6, 10 ** 7 - 1, 10 ** 7, 10 ** 8 - 1, 10 ** 8, 10 ** 9 - 1,
           10 ** 9, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
VIEW_CONFIGS = [(21, 7, 64), (32, 9, 64), (33, 9, 64), (64, 12, 64)]
SHAPES = [(2, 2), (3, 200), (70, 5), (63, 66), (64, 64), (65, 65), (256, 256), (1026, 1026)]
JOINS = [(1, MAX, 2 ** 31, MAX), (2 ** 31, MAX, 0, 0), (10 ** 9, 2 ** 32 - 2, 1, 9), (2 ** 32 - 1, MAX, 2 ** 32 - 1, MAX)]
RANGE_PAIRS = [(2 ** 31 - 1, 2 ** 31), (2 ** 31, MAX), (2 ** 32 - 1, MAX), (1, 2 ** 32 - 2), (1, MAX), (2, 9), (10, 99),
               (63, 65), (255, 1025), (65535, 65536), (10 ** 5 - 1, 10 ** 9), (10 ** 9, 2 ** 31 - 1), (2 ** 32 - 2, 2 ** 32 - 1)]
SPECTRA = [2, 3, 4, 64, 1024, 1025, 1026, 65536, 65537, 65538, 1 << 20]


class Chosen:
    """About 6000 canonical k-mers with the oracle's bins; key i of the (bin, key) order has count P[i % 37] in
    result A and P[(i // 37) % 37] in result B, one key in 8 is in A only and one in 8 in B only."""

    def __init__(self, k, m, B):
        self.k, self.m, self.B = k, m, B
        rng = np.random.default_rng(4000 + k)
        ref = oracle.OracleResult(keys_fasta(*random_keys(rng, k, 6000), k), k, m, B)
        self.nbins = ref.nbins
        keys = OracleTable(ref, ref.nbins)
        n = len(keys)
        assert n >= 5900 and ref.nbins == B and int(keys.count.max()) <= 2
        i = np.arange(n)
        P = np.array(PALETTE, dtype=np.uint64)
        in_a, in_b = i % 8 != 3, i % 8 != 5
        sub = lambda keep, c: Table(keys.hi[keep], keys.lo[keep], c[keep], keys.bin[keep])
        self.a, self.b = sub(in_a, P[i % 37]), sub(in_b, P[(i // 37) % 37])
        self.pair = Pair.of_tables(self.a, self.b, k, m, B, self.nbins)
        self.check_coverage()

    def check_coverage(self):
        p = self.pair
        both = (p.ca > 0) & (p.cb > 0)
        pairs = set(zip(p.ca[both].tolist(), p.cb[both].tolist()))
        assert pairs == {(x, y) for x in PALETTE for y in PALETTE}, "all 37 x 37 pairs of counts"
        assert set(p.ca[p.cb == 0].tolist()) == set(PALETTE) and set(p.cb[p.ca == 0].tolist()) == set(PALETTE)
        assert abs(8 * (p.cb == 0).sum() - len(p.ca)) <= 8 and abs(8 * (p.ca == 0).sum() - len(p.ca)) <= 8
        for rows, cols in SHAPES:
            M = p.matrix(rows, cols)
            assert M[0, 0] == 0 and int(M.sum()) == len(p.ca)
            r, c = min(rows - 1, 64), min(cols - 1, 64)
            assert min(r, c) < 2 or M[1:r, 1:c].any(), "inside the 64 x 64 tile"
            assert M[rows - 1].any() and M[:, cols - 1].any() and M[rows - 1, cols - 1] > 0, "the last row and column"
            for edge in (63, 64):
                if rows > edge + 1:
                    assert M[edge].any(), f"row {edge} of {rows} x {cols}"
                if cols > edge + 1:
                    assert M[:, edge].any(), f"column {edge} of {rows} x {cols}"
            assert rows <= 66 or M[65:rows - 1].any(), "rows beyond the tile"
            assert cols <= 66 or M[:, 65:cols - 1].any(), "columns beyond the tile"
            assert min(rows, cols) <= 66 or M[65:rows - 1, 65:cols - 1].any()
        for side in (0, 1):
            for rg in JOINS:
                assert p.sizes(side, rg).sum() > 0, (side, rg)
        assert (np.bincount(self.a.bin, minlength=self.nbins) > 0).all()  # 64 bins of ~80 keys: none is empty
        last = np.array([self.a.count[j] for j in self.a.last])
        assert (last >= 10 ** 9).any() and (last < 10).any(), "bins ending on a long count and on a short one"

    def profile_reads(self):
        """Reads over A's keys: one read a stored k-mer (every other one on the reverse strand), 4, 5 and 300 stored
        k-mers joined back to back (the windows across a joint are random k-mers) and joined by an N (only the
        stored windows are valid), and random reads."""
        k, t = self.k, self.a
        rng = np.random.default_rng(5000 + k)
        fwd = key_bases(t.hi, t.lo, k)
        rh, rl = revcomp(t.hi, t.lo, k)
        rev = key_bases(rh, rl, k)
        reads = [(rev if i % 2 else fwd)[i].tobytes() for i in range(len(t))]
        for n in (4, 5, 300):
            for sep in (b"", b"N"):
                for _ in range(6):
                    reads.append(sep.join(reads[j] for j in rng.integers(0, len(t), n)))
        reads += [_rand_read(rng, int(rng.integers(0, 200))) for _ in range(100)]
        return csr(reads)


@functools.lru_cache(maxsize=None)
def chosen(k, m, B):
    return Chosen(k, m, B)


# ---- part 3: read statistics of chosen count arrays
STAT_WINDOWS = [0, 1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 300, 1000]
STAT_RANGES = [(1, MAX), (2 ** 31, MAX)]


def _stat_values(rng, w):
    """The value patterns of one window count w: a list of uint32 arrays of w entries."""
    out = [np.full(w, 7, dtype=np.uint32), np.full(w, MAX, dtype=np.uint32), np.zeros(w, dtype=np.uint32),
           rng.integers(0, 2 ** 32, w, dtype=np.uint64).astype(np.uint32)]
    out += [rng.integers(0, 4, w, dtype=np.uint64).astype(np.uint32),                    # many ties
            rng.integers(2 ** 31 - 2, 2 ** 31 + 2, w, dtype=np.uint64).astype(np.uint32),  # around bit 31
            rng.integers(65534, 65539, w, dtype=np.uint64).astype(np.uint32),              # around bit 16
            np.where(np.arange(w) % 2 == 0, 0, MAX).astype(np.uint32),                     # the two ends, alternating
            np.full(w, 2 ** 31, dtype=np.uint32), (np.arange(w) % 7).astype(np.uint32)]
    step = max((2 ** 32 - 1) // max(w, 1), 1)
    asc = (np.arange(w, dtype=np.uint64) * np.uint64(step)).astype(np.uint32)
    out += [asc, asc[::-1].copy()]
    for b in (0, 1, 15, 16, 30, 31):
        a = np.uint32(0x2A54 & ~(1 << b)) if b < 30 else np.uint32(5)
        for n_hi in sorted({0, 1, (w - 1) // 2, (w + 1) // 2, w // 2 + 1, w - 1} & set(range(w + 1))):
            v = np.full(w, a, dtype=np.uint32)
            v[rng.permutation(w)[:n_hi]] |= np.uint32(1 << b)  # n_hi of w hold the bit: the median on either side
            out.append(v)
    if w:
        for at, x in ((0, MAX), (w - 1, MAX), (0, 0), (w - 1, 0)):  # one outlier at either end
            v = np.full(w, 1000, dtype=np.uint32)
            v[at] = x
            out.append(v)
    return out


def stat_batch(k, seed, only=None):
    """(counts, valid, offsets) by position for the reads of part 3: every window count x value pattern x valid mask
    (1: all ones, 2: random halves, 3: none valid, 4 / 5: only below / only above window 256), shuffled so that every
    wave of a workgroup meets every shape.  A read of w windows has w + k - 1 positions (w = 0: k - 1 or 0); the k - 1
    positions behind the last window hold values that must not count."""
    rng = np.random.default_rng(seed)
    reads = []
    for w in STAT_WINDOWS:
        for v in _stat_values(rng, w):
            for mask in (1, 2, 3, 4, 5):
                if mask >= 4 and w <= 256:
                    continue
                ok = np.ones(w, dtype=np.uint8)
                if mask == 2:
                    ok = (rng.random(w) < 0.5).astype(np.uint8)
                elif mask == 3:
                    ok[:] = 0
                elif mask == 4:
                    ok[256:] = 0
                elif mask == 5:
                    ok[:256] = 0
                reads.append((v, ok))
    order = rng.permutation(len(reads))
    if only is not None:
        order = order[:only]
    counts, valid, lens = [], [], []
    for j in order:
        v, ok = reads[j]
        pad = k - 1 if (len(v) or j % 2) else 0
        counts += [v, np.full(pad, 0xDEADBEEF, dtype=np.uint32)]
        valid += [ok, np.ones(pad, dtype=np.uint8)]
        lens.append(len(v) + pad)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    return cat(counts, np.uint32), cat(valid, np.uint8), offsets


def expected_select(counts, valid, offsets, k, lo=1, hi=MAX):
    """fk_read_stat of every read: np.sort over the valid windows (valid None: every existing window), the median
    element (w - 1) // 2, the sum in uint64."""
    n = len(counts)
    lens = np.diff(offsets.astype(np.int64))
    end = np.repeat(offsets[1:].astype(np.int64), lens)
    exists = np.arange(n) + k <= end
    eff = exists if valid is None else exists & (valid != 0)
    return expected_stats(counts, eff.astype(np.uint8), offsets, lo, hi)
