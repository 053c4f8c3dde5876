"""fk_spectrum* and the count-range views (fk_bin_sizes_range / fk_get_bin_range / fk_write_bins_range)
against the CPU oracle, through the C-ABI only (needs a GPU).  Everything is exact.

Expectations come from oracle.OracleResult.bin_arrays (query_util.OracleTable): the spectrum is
np.bincount(np.minimum(count, n - 1), minlength=n), a range view is a boolean mask.  For use_ht = 1 the
order inside a bin is the table's, so a filtered bin is compared with the context's own unfiltered
fk_get_bin / fk_write_bins output masked (order preserved) and, sorted, with the oracle's.

Inputs: `small` (3000 reads of a 200 kb genome: 62 % singletons at k = 28, counts up to 7), `spiky`
(small + 3000 identical reads + 2000 poly-A reads: a group of k-mers at count exactly 3000 and one
k-mer above 90 000, either side of any LDS bound and of the last exact entry), `heavy` (60 000 reads of
a 3 Gb genome + the same repeats: 4.3 M distinct k-mers at k = 28, 99.9 % singletons, buckets split
into sub-buckets and staged pieces)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import fastkmer_amd as fk
import oracle
from query_util import CONFIGS, OracleTable, pack
from test_gpu_query import REP

pytestmark = pytest.mark.gpu

MAX = fk.MAX_COUNT
POLY = b"".join(b">p%d\n" % i + b"A" * 100 + b"\n" for i in range(2_000))
RANGES = [(1, MAX), (2, MAX), (1, 1), (2, 3), (3000, 3000), (8, MAX), (4_000_000_000, MAX)]


class Job:
    """An input with the oracle's result over it."""

    def __init__(self, fasta, k, m, B, threads=1):
        self.fasta, self.k, self.m, self.B = fasta, k, m, B
        self.ref = oracle.OracleResult(fasta, k, m, B, threads=threads)
        self.tab = OracleTable(self.ref, self.ref.nbins)
        self.nbins = self.ref.nbins
        self.count = self.tab.count

    def spectrum(self, n, mine=None):
        """(hist, tail k-mers) of the k-mers selected by `mine` (all)."""
        c = self.count if mine is None else self.count[mine]
        c = c.astype(np.int64)
        return (np.bincount(np.minimum(c, n - 1), minlength=n).astype(np.uint64), int(c[c >= n - 1].sum()))

    def sizes(self, lo, hi, mine=None):
        keep = (self.count >= lo) & (self.count <= hi)
        if mine is not None:
            keep &= mine
        return np.bincount(self.tab.bin[keep], minlength=self.nbins).astype(np.uint64)

    def bin(self, b, lo=1, hi=MAX):
        """(keys in fk_get_bin's layout, counts) of bin b filtered to [lo, hi]."""
        h, l, c = self.ref.bin_arrays(b)
        keep = (c >= lo) & (c <= hi)
        return pack(h[keep], l[keep], self.k), c[keep]


@functools.lru_cache(maxsize=None)
def small(k, m, B):
    return Job(fk.synth_fasta(3000, 100, 200_000, seed=0xA0 + k), k, m, B)


@functools.lru_cache(maxsize=None)
def spiky(k, m):
    return Job(fk.synth_fasta(3000, 100, 200_000, seed=0xA0 + k) + REP + POLY, k, m, 64)


@functools.lru_cache(maxsize=None)
def heavy(k, m):
    return Job(fk.synth_fasta(60_000, 100, 3_000_000_000, seed=0xC1 + k) + REP + POLY, k, m, 16, threads=4)


def run_counter(job, **kw):
    kc = fk.KmerCounter(job.k, job.m, 3, job.B, **kw)
    kc.ingest(job.fasta)
    kc.finish()
    return kc


@pytest.fixture(scope="module")
def counted():
    """Counted jobs shared by the tests that only read a result: counted(job, use_ht) -> KmerCounter."""
    cache = {}

    def get(job, use_ht=False):
        key = (id(job), bool(use_ht))
        if key not in cache:
            cache[key] = run_counter(job, use_ht=use_ht)
        return cache[key]

    yield get
    for kc in cache.values():
        kc.close()


def check_spectrum(kc, job, n, mine=None):
    want, want_tail = job.spectrum(n, mine)
    got, tail = kc.spectrum(n, return_tail=True)
    assert got.dtype == np.uint64 and len(got) == n and got[0] == 0
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"n={n}: entries {bad[:5]} are {got[bad[:5]]}, the oracle has {want[bad[:5]]}"
    assert tail == want_tail, f"n={n}: tail k-mers {tail} != {want_tail}"
    assert np.array_equal(kc.spectrum(n), want)  # tail_kmers = NULL
    return got, tail


def sorted_bin(keys, counts, k):
    """A bin's (keys, counts) in ascending key order."""
    kw = 2 if k > 32 else 1
    rows = keys.reshape(-1, kw)
    o = np.lexsort((rows[:, -1], rows[:, 0]))
    return rows[o].reshape(-1), counts[o]


def check_bin(kc, job, b, lo, hi):
    """get_bin(b) filtered to [lo, hi] against the kernel-independent expectation."""
    kw = 2 if job.k > 32 else 1
    keys, counts = kc.get_bin(b, min_count=lo, max_count=hi)
    want_keys, want_counts = job.bin(b, lo, hi)
    if kc.use_ht:
        ukeys, ucounts = kc.get_bin(b)  # the context's own unfiltered bin, masked: order preserved
        keep = (ucounts >= lo) & (ucounts <= hi)
        assert np.array_equal(keys, ukeys.reshape(-1, kw)[keep].reshape(-1)), f"bin {b} [{lo}, {hi}]: keys / order"
        assert np.array_equal(counts, ucounts[keep]), f"bin {b} [{lo}, {hi}]: counts / order"
        keys, counts = sorted_bin(keys, counts, job.k)
    assert np.array_equal(keys, want_keys), f"bin {b} [{lo}, {hi}]: keys differ from the oracle's"
    assert np.array_equal(counts, want_counts), f"bin {b} [{lo}, {hi}]: counts differ from the oracle's"
    return len(counts)


# 1. the spectrum of a skewed input, every configuration and both count modes
@pytest.mark.parametrize("use_ht", [False, True])
@pytest.mark.parametrize("k,m,B", CONFIGS)
def test_spectrum_small(counted, k, m, B, use_ht):
    job = small(k, m, B)
    assert job.ref.distinct > 50_000 and (job.count == 1).mean() > 0.5 and 2 < job.count.max() < 4096
    kc = counted(job, use_ht)
    st = kc.stats()
    for n in (2, 3, 8, 4096):
        hist, tail = check_spectrum(kc, job, n)
        assert int(hist.sum()) == st["distinct"] == job.ref.distinct
        assert int((np.arange(n - 1, dtype=np.uint64) * hist[:n - 1]).sum()) + tail == st["kmers"] == job.ref.total_kmers


# 2. counts far above any table: 3000 and the maximum on either side of the last exact entry
@pytest.mark.parametrize("use_ht", [False, True])
@pytest.mark.parametrize("k,m", [(28, 10), (55, 12)])
def test_spectrum_spiky(counted, k, m, use_ht):
    job = spiky(k, m)
    top = int(job.count.max())
    assert top >= 90_000 and (job.count == 3000).sum() > 1 and (job.count == top).sum() == 1
    kc = counted(job, use_ht)
    for n in (2, 3, 8, 9, 10, 11, 64, 1023, 1024, 1025, 1026, 3000, 3001, 3002, 4096, top + 1, top + 2, 1 << 18):
        hist, tail = check_spectrum(kc, job, n)
        assert int(hist.sum()) == job.ref.distinct
    hist = kc.spectrum(top + 2)
    assert hist[3000] == (job.count == 3000).sum() and hist[top] == 1 and hist[top + 1] == 0


# ... and through the kernel of results of 2^32 k-mers and more (64-bit LDS entries; a test hook)
def test_spectrum_spiky_wide_table(monkeypatch):
    monkeypatch.setenv("FASTKMER_DEBUG_SPECTRUM_WIDE", "1")
    job = spiky(28, 10)
    with run_counter(job) as kc:
        for n in (2, 8, 9, 10, 1024, 4096, int(job.count.max()) + 2):
            check_spectrum(kc, job, n)


# 3. heavy buckets split into sub-buckets, and a job counted from staged pieces
def check_heavy(kc, job):
    for n in (4, 4096):
        check_spectrum(kc, job, n)
    assert np.array_equal(kc.bin_sizes(min_count=2), job.sizes(2, MAX))
    for b in range(job.nbins):
        check_bin(kc, job, b, 2, MAX)


@pytest.mark.parametrize("k,m", [(28, 10), (55, 12)])
def test_heavy_split_buckets(monkeypatch, k, m):
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2600")
    job = heavy(k, m)
    assert job.ref.distinct > 2_000_000 and (job.count == 1).mean() > 0.99
    with run_counter(job) as kc:
        st = kc.stats()
        assert st["split_buckets"] > 100 and st["kmers"] == job.ref.total_kmers, st
        check_heavy(kc, job)


def test_heavy_staged_pieces(monkeypatch):
    import torch
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", "2600")
    monkeypatch.setenv("FASTKMER_INGEST_SEG", str(262144))
    monkeypatch.setenv("FASTKMER_PIECE_BYTES", str(524288))
    job = heavy(28, 10)
    host = torch.frombuffer(bytearray(job.fasta), dtype=torch.uint8).pin_memory()
    with fk.KmerCounter(28, 10, 3, 16) as kc:
        kc.ingest_ptr(host.data_ptr(), host.numel())
        kc.finish()
        st = kc.stats()
        assert st["pieces_counted"] == 4 and st["kmers"] == job.ref.total_kmers, st
        check_heavy(kc, job)


# 4. range views
def check_ranges(kc, job, need_singleton_bin):
    unfiltered = kc.bin_sizes()
    assert np.array_equal(unfiltered, job.sizes(1, MAX))
    ones = job.sizes(1, 1)
    only_singletons = np.nonzero((unfiltered > 0) & (ones == unfiltered))[0]
    assert len(only_singletons) > 0 or not need_singleton_bin
    nonempty = np.nonzero(unfiltered)[0]
    bins = [int(nonempty[0]), int(np.argmax(unfiltered)), job.nbins - 1]
    if len(only_singletons):
        bins.append(int(only_singletons[0]))
    kept_any = 0
    for lo, hi in RANGES:
        sizes = kc.bin_sizes(min_count=lo, max_count=None if hi == MAX else hi)
        want = job.sizes(lo, hi)
        assert np.array_equal(sizes, want), f"[{lo}, {hi}]: bins {np.nonzero(sizes != want)[0][:5]} differ"
        for b in bins:
            assert check_bin(kc, job, b, lo, hi) == want[b]
        kept_any += int(want.sum() > 0)
    assert kept_any >= 4  # the ranges are not all empty on this input
    assert not job.sizes(4_000_000_000, MAX).any()
    # (1, MAX) through the range calls themselves equals the unfiltered calls
    L, kw = fk.lib(), 2 if job.k > 32 else 1
    raw = np.zeros(job.nbins, dtype=np.uint64)
    assert L.fk_bin_sizes_range(kc._h, 1, MAX, raw.ctypes.data) == 0 and np.array_equal(raw, unfiltered)
    n = ctypes.c_size_t(0)
    for b in bins:
        ukeys, ucounts = kc.get_bin(b)
        cap = max(len(ucounts), 1)
        keys, counts = np.zeros(cap * kw, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
        assert L.fk_get_bin_range(kc._h, b, 1, MAX, keys.ctypes.data, counts.ctypes.data, cap, ctypes.byref(n)) == 0
        assert n.value == len(ucounts)
        assert np.array_equal(keys[:n.value * kw], ukeys) and np.array_equal(counts[:n.value], ucounts)
    # the buffer rules (fk_get_bin's): cap = n - 1 is refused with *n set; NULL keys still fills counts
    b = int(np.argmax(job.sizes(2, MAX)))
    want_n = int(job.sizes(2, MAX)[b])
    assert want_n > 1
    keys, counts = np.zeros(want_n * kw, dtype=np.uint64), np.full(want_n, 77, dtype=np.uint32)
    n.value = 0
    assert L.fk_get_bin_range(kc._h, b, 2, MAX, keys.ctypes.data, counts.ctypes.data, want_n - 1, ctypes.byref(n)) == -6
    assert n.value == want_n and not keys.any() and (counts == 77).all()
    n.value = 0
    assert L.fk_get_bin_range(kc._h, b, 2, MAX, None, counts.ctypes.data, want_n, ctypes.byref(n)) == 0
    full_keys, full_counts = kc.get_bin(b, min_count=2)
    assert n.value == want_n and np.array_equal(counts, full_counts)
    n.value = 0
    assert L.fk_get_bin_range(kc._h, b, 2, MAX, keys.ctypes.data, None, want_n, ctypes.byref(n)) == 0
    assert n.value == want_n and np.array_equal(keys, full_keys)
    n.value = 0
    assert L.fk_get_bin_range(kc._h, b, 2, MAX, None, None, want_n, ctypes.byref(n)) == 0 and n.value == want_n
    n.value = 0
    assert L.fk_get_bin_range(kc._h, b, 2, MAX, None, None, 0, ctypes.byref(n)) == -6 and n.value == want_n
    for bad in (-1, job.nbins):
        assert L.fk_get_bin_range(kc._h, bad, 2, MAX, None, None, 0, ctypes.byref(n)) == -6


@pytest.mark.parametrize("use_ht", [False, True])
@pytest.mark.parametrize("k,m,B", CONFIGS)
def test_range_views_small(counted, k, m, B, use_ht):
    job = small(k, m, B)
    assert not job.sizes(8, MAX).any()  # an empty range on this input
    check_ranges(counted(job, use_ht), job, need_singleton_bin=(k, m, B) in [(28, 10, 2048), (55, 12, 8192)])


@pytest.mark.parametrize("use_ht", [False, True])
@pytest.mark.parametrize("k,m", [(28, 10), (55, 12)])
def test_range_views_spiky(counted, k, m, use_ht):
    job = spiky(k, m)
    assert job.sizes(3000, 3000).sum() > 1 and job.sizes(8, MAX).sum() > job.sizes(3000, 3000).sum()
    check_ranges(counted(job, use_ht), job, need_singleton_bin=False)


# 5. bin files of a range
def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))} if os.path.isdir(d) else {}


def _filter_files(files, lo, hi, eof):
    """Bin files with the lines out of [lo, hi] removed; the trailer only where a line remains."""
    out = {}
    for name, text in files.items():
        body = text[:-3] if text.endswith(b"EOF") else text
        kept = [ln for ln in body.splitlines(keepends=True) if lo <= int(ln.split(b"\t")[1]) <= hi]
        if kept:
            out[name] = b"".join(kept) + (b"EOF" if eof else b"")
    return out


@pytest.mark.parametrize("use_ht", [False, True])
def test_write_bins_with_a_range(counted, tmp_path, use_ht):
    job = small(28, 10, 2048)
    kc = counted(job, use_ht)
    job.ref.write_bins(str(tmp_path / "ref"), sorted_eof=not use_ht)
    ref_files = _files(tmp_path / "ref")
    kc.write_bins(str(tmp_path / "all"))
    own_files = _files(tmp_path / "all")
    assert sorted(own_files) == sorted(ref_files) and len(ref_files) > 2000
    for lo, hi in ((2, MAX), (1, 1)):
        d = tmp_path / f"r{lo}_{hi}"
        kc.write_bins(str(d), min_count=lo, max_count=None if hi == MAX else hi)
        got = _files(d)
        want = _filter_files(ref_files, lo, hi, eof=not use_ht)
        assert sorted(got) == sorted(want) == [f"bin{b}" for b in sorted(np.nonzero(job.sizes(lo, hi))[0], key=str)]
        assert len(got) < len(ref_files)  # some bins have no kept line, so no file
        if not use_ht:
            bad = [f for f in want if got[f] != want[f]]
            assert not bad, f"[{lo}, {hi}]: {len(bad)} files differ from the oracle's filtered, e.g. {bad[:3]}"
            assert all(t.endswith(b"\nEOF") for t in got.values())
        else:  # table order: the context's own unfiltered files filtered, and the oracle's lines as a set
            own = _filter_files(own_files, lo, hi, eof=False)
            bad = [f for f in own if got[f] != own[f]]
            assert not bad, f"[{lo}, {hi}]: {len(bad)} files lost the table order, e.g. {bad[:3]}"
            assert all(sorted(got[f].splitlines()) == sorted(want[f].splitlines()) for f in want)
            assert not any(t.endswith(b"EOF") for t in got.values())
    singles_only = int(((job.sizes(1, MAX) > 0) & (job.sizes(2, MAX) == 0)).sum())
    assert singles_only > 0 and len(_files(tmp_path / f"r2_{MAX}")) == len(ref_files) - singles_only
    # (1, MAX) through the range call reproduces fk_write_bins byte for byte
    assert fk.lib().fk_write_bins_range(kc._h, str(tmp_path / "same").encode(), 1, MAX) == 0
    assert _files(tmp_path / "same") == own_files
    # a range that keeps nothing writes no file
    kc.write_bins(str(tmp_path / "none"), min_count=8)
    assert _files(tmp_path / "none") == {}


# ... and through the CLI's environment variables (the positional contract untouched)
def test_cli_count_range_and_spectrum(tmp_path):
    import subprocess
    job = spiky(28, 10)
    inp = tmp_path / "in.fa"
    inp.write_bytes(job.fasta)
    job.ref.write_bins(str(tmp_path / "ref"))
    ref_files = _files(tmp_path / "ref")
    base = {k: v for k, v in os.environ.items() if not k.startswith("FASTKMER_CLI_")}

    def run(prefix, write, **env):
        r = subprocess.run([fk.CLI_PATH, "28", "10", "3", "64", "0", "0", str(inp), str(tmp_path) + "/", prefix,
                            str(write), "0", "0"], capture_output=True, text=True, env=dict(base, **env))
        assert r.returncode == 0, r.stderr
        return _files(tmp_path / f"{prefix}k28_m10_x3_b64_s0"), r.stdout

    def spectrum_text(n):
        hist = job.spectrum(n)[0]
        return "".join(f"{'>=' if c == n - 1 else ''}{c}\t{int(hist[c])}\n" for c in range(1, n) if hist[c]).encode()

    plain, out = run("plain_", 1)  # none of the variables: as before
    assert plain == ref_files and "Spectrum" not in out
    got, out = run("both_", 1, FASTKMER_CLI_MIN_COUNT="2", FASTKMER_CLI_MAX_COUNT="3000", FASTKMER_CLI_SPECTRUM="3002")
    want = _filter_files(ref_files, 2, 3000, eof=True)
    want["spectrum.txt"] = spectrum_text(3002)
    assert got == want and b"\n3000\t" in got["spectrum.txt"] and b"\n>=3001\t1\n" in got["spectrum.txt"]
    got, _ = run("min_", 1, FASTKMER_CLI_MIN_COUNT="3000")
    assert got == _filter_files(ref_files, 3000, MAX, eof=True) and 0 < len(got) < len(ref_files)
    got, _ = run("spec_", 0, FASTKMER_CLI_SPECTRUM="8", FASTKMER_CLI_MIN_COUNT="2")  # write = 0: the spectrum only
    assert got == {"spectrum.txt": spectrum_text(8)} and got["spectrum.txt"].splitlines()[-1].startswith(b">=7\t")


# 6. the device form on the caller's stream
def test_spectrum_ptr_on_the_callers_stream():
    import torch
    job = spiky(28, 10)
    for stream in (None, torch.cuda.Stream()):  # torch's default stream, then a side stream
        with run_counter(job) as kc:  # closed before the stream goes away
            with torch.cuda.stream(stream):
                kc.set_stream(torch.cuda.current_stream().cuda_stream)
                for n in (2, 4096):
                    want, want_tail = kc.spectrum(n, return_tail=True)
                    assert np.array_equal(want, job.spectrum(n)[0]) and want_tail == job.spectrum(n)[1]
                    d_hist = torch.full((n,), -7, dtype=torch.int64, device="cuda")
                    d_tail = torch.full((1,), -7, dtype=torch.int64, device="cuda")
                    d_only = torch.full((n,), 1 << 40, dtype=torch.int64, device="cuda")
                    for _ in range(2):  # overwritten, not accumulated into
                        kc.spectrum_ptr(d_hist.data_ptr(), n, d_tail.data_ptr())
                        kc.spectrum_ptr(d_only.data_ptr(), n)
                    torch.cuda.current_stream().synchronize()
                    assert np.array_equal(d_hist.cpu().numpy().view(np.uint64), want)
                    assert np.array_equal(d_only.cpu().numpy().view(np.uint64), want)
                    assert int(d_tail.cpu().numpy().view(np.uint64)[0]) == want_tail


# 7. states, arguments, an empty job, the other readers of the result
def _raw_calls(kc, out_dir, n=8, lo=2, hi=MAX):
    """The five C calls' return codes."""
    import torch
    L = fk.lib()
    hist = np.zeros(max(n, 1), dtype=np.uint64)
    d_hist = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
    sizes = np.zeros(kc.num_bins, dtype=np.uint64)
    cnt = ctypes.c_size_t(0)
    rcs = [L.fk_spectrum(kc._h, hist.ctypes.data, n, None),
           L.fk_spectrum_device(kc._h, ctypes.c_void_p(d_hist.data_ptr()), n, None),
           L.fk_bin_sizes_range(kc._h, lo, hi, sizes.ctypes.data),
           L.fk_get_bin_range(kc._h, 0, lo, hi, None, None, 1 << 40, ctypes.byref(cnt)),
           L.fk_write_bins_range(kc._h, str(out_dir).encode(), lo, hi)]
    torch.cuda.synchronize()
    return rcs


def test_states_arguments_and_an_empty_job(tmp_path):
    job = small(28, 10, 2048)
    d = tmp_path / "out"
    with fk.KmerCounter(28, 10, 3, 2048) as kc:
        assert _raw_calls(kc, d) == [-2] * 5  # FK_E_STATE: nothing counted yet
        kc.ingest(job.fasta)
        assert _raw_calls(kc, d) == [-2] * 5
        kc.finish()
        assert _raw_calls(kc, d) == [0] * 5
        check_spectrum(kc, job, 8)
        # FK_E_INVALID: n = 1 (the spectrum calls), min_count = 0, min > max (the range calls)
        assert _raw_calls(kc, d, n=1)[:2] == [-1, -1] and _raw_calls(kc, d, n=0)[:2] == [-1, -1]
        assert _raw_calls(kc, d, lo=0)[2:] == [-1, -1, -1]
        assert _raw_calls(kc, d, lo=3, hi=2)[2:] == [-1, -1, -1]
        for call in (lambda: kc.spectrum(1), lambda: kc.bin_sizes(min_count=0), lambda: kc.get_bin(0, min_count=5, max_count=4),
                     lambda: kc.write_bins(str(d), min_count=0)):
            with pytest.raises(fk.FastKmerError) as e:
                call()
            assert e.value.code == -1
        L = fk.lib()
        assert L.fk_spectrum(kc._h, None, 8, None) == -1 and L.fk_bin_sizes_range(kc._h, 1, MAX, None) == -1
        assert L.fk_get_bin_range(kc._h, 0, 1, MAX, None, None, 0, None) == -1
        assert L.fk_write_bins_range(kc._h, None, 1, MAX) == -1
        kc.ingest_chunk(job.fasta[:114 * 10], last=False)  # a new job's first ingest drops the result
        assert _raw_calls(kc, d) == [-2] * 5
        kc.ingest_chunk(job.fasta[114 * 10:], last=True)
        kc.finish()
        assert _raw_calls(kc, d) == [0] * 5
        check_spectrum(kc, job, 8)
        assert np.array_equal(kc.bin_sizes(min_count=2), job.sizes(2, MAX))
    for use_ht in (False, True):
        with fk.KmerCounter(28, 10, 3, 2048, use_ht=use_ht) as kc:  # an empty job answers, with zeros
            kc.ingest(b"")
            kc.finish()
            e = tmp_path / f"empty{int(use_ht)}"
            assert _raw_calls(kc, e) == [0] * 5
            hist, tail = kc.spectrum(16, return_tail=True)
            assert not hist.any() and tail == 0 and len(hist) == 16
            assert not kc.bin_sizes(min_count=2).any() and len(kc.get_bin(0, min_count=2)[1]) == 0
            assert _files(e) == {}


def test_the_new_calls_only_read_the_result(tmp_path):
    job = small(28, 10, 2048)
    with run_counter(job) as kc:  # its own context: fk_get_bin before any fk_write_bins
        keys = pack(job.tab.hi, job.tab.lo, job.k)
        some = np.nonzero(job.sizes(1, MAX))[0][[0, 7, -1]].tolist()

        def readers():
            q = kc.query(keys, return_bins=True)
            return [q[0], q[1]] + [a for b in some for a in kc.get_bin(b)]

        before = readers()
        assert np.array_equal(before[0], job.count) and np.array_equal(before[1], job.tab.bin)
        kc.spectrum(4096), kc.spectrum(2), kc.bin_sizes(min_count=2)
        for b in some:
            kc.get_bin(b, min_count=2), kc.get_bin(b, min_count=1, max_count=1)
        after = readers()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        kc.write_bins(str(tmp_path / "r"), min_count=2)
        after = readers()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        kc.write_bins(str(tmp_path / "all"))  # materialises the dense copy; the range views still walk the buckets
        check_spectrum(kc, job, 8)
        for b in some:
            check_bin(kc, job, b, 2, MAX)
        after = readers()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        job.ref.write_bins(str(tmp_path / "ref"))
        assert _files(tmp_path / "all") == _files(tmp_path / "ref")


# 8. ranks: a rank's spectrum and sizes cover the bins it owns; the ranks' sum is the job's
def check_ranks(ranks, job, owner):
    total = np.zeros(4096, dtype=np.uint64)
    total_tail = 0
    sizes = np.zeros(job.nbins, dtype=np.uint64)
    for r, kc in enumerate(ranks):
        mine = owner[job.tab.bin] == r
        assert mine.any() and not mine.all()
        for n in (2, 8):
            check_spectrum(kc, job, n, mine)
        hist, tail = check_spectrum(kc, job, 4096, mine)
        total += hist
        total_tail += tail
        s = kc.bin_sizes(min_count=2)
        assert not s[owner != r].any(), f"rank {r} reports sizes for bins it does not own"
        assert np.array_equal(s, job.sizes(2, MAX, mine))
        other = int(np.nonzero((owner != r) & (job.sizes(2, MAX) > 0))[0][0])
        assert len(kc.get_bin(other, min_count=2)[1]) == 0
        own = int(np.nonzero((owner == r) & (job.sizes(2, MAX) > 0))[0][0])
        check_bin(kc, job, own, 2, MAX)
        sizes += s
    want, want_tail = job.spectrum(4096)
    assert np.array_equal(total, want) and total_tail == want_tail
    assert np.array_equal(sizes, job.sizes(2, MAX))


def test_ranks_two_exchanging():
    from test_gpu_comm import record_shards, run_local_job
    job = small(28, 10, 2048)
    ctxs = run_local_job(record_shards(job.fasta, 2), 28, 10, 3, 2048)
    try:
        owner = ctxs[0].bin_owners()
        assert np.array_equal(owner, np.arange(2048) % 2)
        check_ranks(ctxs, job, owner)
    finally:
        for kc in ctxs:
            kc.close()


def test_ranks_three_with_lpt_owners():
    import torch
    k, m, B, G = 28, 10, 2048, 3
    job = small(k, m, B)
    shards = [job.fasta[r * 114 * 1000:(r + 1) * 114 * 1000] for r in range(G)]
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
        check_ranks(ranks, job, np.asarray(owner))
    finally:
        for kc in ranks:
            kc.close()
