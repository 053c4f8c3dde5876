"""The fold of landed pieces into weighted keys, through the C-ABI.

A staged piece that is not the job's last is folded while the rest of the input lands: its
duplicate k-mers become weighted keys (k <= 30: the four bits above the k-mer hold weight - 1, one
entry stands for 1..15 occurrences), and every tier of the count adds weights where it added 1.
A bin's multiset is unchanged by that, so every result here is bit-exact against the CPU oracle
(or against the same job with the fold off).  The pieces are made small (FASTKMER_PIECE_BYTES) as
in test_gpu_pieces, FASTKMER_FOLD=2 folds every eligible piece whatever the first piece's sample
says, and FASTKMER_DEBUG_FOLD_WMAX lowers the weight cap so that small inputs cross it.
"""
import functools

import numpy as np
import pytest

import fastkmer_amd as fk
import oracle
from test_gpu_parity import assert_same_as_oracle
from test_gpu_pieces import count_pinned

pytestmark = pytest.mark.gpu
F = 11


@pytest.fixture
def small_pieces(monkeypatch):
    monkeypatch.setenv("FASTKMER_INGEST_SEG", str(256 << 10))
    monkeypatch.setenv("FASTKMER_PIECE_BYTES", str(512 << 10))


@pytest.fixture
def forced(small_pieces, monkeypatch):
    monkeypatch.setenv("FASTKMER_FOLD", "2")


# inputs and their oracle results, computed once and shared (never modified)
@functools.lru_cache(maxsize=None)
def reads_20x():
    return fk.synth_fasta(40_000, 100, 200_000, seed=0xF01D)  # 40,000 reads of 100 bp, a 200 kbp genome


@functools.lru_cache(maxsize=None)
def skewed():
    # test_piece_counts_disjoint_and_skewed_pieces's input: two unrelated genomes, one read repeated
    # 6,000 times (multiplicities far above the weight cap) and a low-complexity stretch whose k-mers
    # are counted above 65535
    a = fk.synth_fasta(12_000, 100, 300_000, seed=0xA2)
    b = fk.synth_fasta(12_000, 100, 300_000, seed=0xA3, first_read=12_000)
    rep = b"".join(b">r%010d\n" % i + b"ACGTTGCAAGGCTTACCGATCGGATTACAGGCATCGATCGGGCTAGCTAGGCTAGCTTACGAGCTAGCATCGACTAGCATG"
                   b"CATGCATCGACGTAGCATCG\n" for i in range(6_000))
    low = b"".join(b">l%d\n" % i + (b"ACACACACAC" * 10) + b"\n" for i in range(6_000))
    return a + rep + b + low + a[:len(a) // 2]


@functools.lru_cache(maxsize=None)
def ref_of(name, k=28, m=10, B=2048):
    return oracle.OracleResult({"reads_20x": reads_20x, "skewed": skewed}[name](), k, m, B)


# ---- one weighted bucket through the wave tier's kernel

def weighted_bucket(rng, k, n, c0, c1):
    """n entries (key | (weight - 1) << 2k) inside cells [c0, c1): the same k-mer under several
    weights, k-mers at both ends of the cell range, weights 1..15."""
    sh = 2 * k - F
    lo, hi = c0 << sh, (c1 << sh) - 1
    ndist = max(1, n // 3)
    ends = np.array([lo, hi], dtype=np.uint64)[:ndist]
    base = np.unique(np.concatenate([ends, rng.integers(lo + 1, hi, ndist - len(ends), dtype=np.uint64)]))
    keys = np.concatenate([base, rng.choice(base, n - len(base))])
    w = rng.integers(1, 16, len(keys)).astype(np.uint64)
    w[:min(2, len(w))] = (15, 1)[:min(2, len(w))]  # both ends of the weight range
    order = rng.permutation(len(keys))
    return keys[order], w[order]


@pytest.mark.parametrize("n", [1, 64, 65, 512])
@pytest.mark.parametrize("k", [28, 30])
def test_weighted_bucket_counts_sum_the_weights(k, n):
    rng = np.random.default_rng(1000 * k + n)
    c0, c1 = 5, 9
    keys, w = weighted_bucket(rng, k, n, c0, c1)
    assert len(keys) == n
    packed = keys | ((w - np.uint64(1)) << np.uint64(2 * k))
    got_k, got_c = fk.debug_wave_count(packed, k, F, c0, c1, 640, weighted=True)
    ek, inv = np.unique(keys, return_inverse=True)
    ec = np.bincount(inv, weights=w.astype(np.float64)).astype(np.int64)
    assert np.array_equal(got_k, ek) and np.array_equal(got_c.astype(np.int64), ec)
    if n >= 64:
        assert len(ek) < n  # a k-mer under several weights


def test_weighted_hook_rejects_a_weight_where_there_is_no_field():
    # k = 31: the key takes 62 bits, nothing above it is a weight
    key = (np.uint64(5) << np.uint64(62 - F)) | (np.uint64(1) << np.uint64(62))
    with pytest.raises(fk.FastKmerError):
        fk.debug_wave_count(np.array([key], dtype=np.uint64), 31, F, 5, 6, 640, weighted=True)
    # k = 28: bits above the four-bit field are no weight either
    key = (np.uint64(5) << np.uint64(56 - F)) | (np.uint64(1) << np.uint64(60))
    with pytest.raises(fk.FastKmerError):
        fk.debug_wave_count(np.array([key], dtype=np.uint64), 28, F, 5, 6, 640, weighted=True)
    # ... and the unweighted hook takes no weight at all
    key = (np.uint64(5) << np.uint64(56 - F)) | (np.uint64(3) << np.uint64(56))
    with pytest.raises(fk.FastKmerError):
        fk.debug_wave_count(np.array([key], dtype=np.uint64), 28, F, 5, 6, 640)


# ---- folded jobs against the oracle

def assert_folded(kc, at_least=1):
    fs = kc.fold_stats()
    assert fs["pieces_folded"] >= at_least, fs
    assert 0 < fs["entries_out"] < fs["entries_in"], fs
    return fs


@pytest.mark.parametrize("B", [2048, 8192])
def test_forced_fold_vs_oracle(forced, B):
    kc = count_pinned(reads_20x(), 28, 10, B, repeat=2)  # twice: the fold's buffers are reused
    st = kc.stats()
    assert st["pieces_counted"] == 4 and st["fused_map"] == 1
    assert_folded(kc)
    ref = ref_of("reads_20x", B=B)
    assert st["kmers"] == ref.total_kmers and st["distinct"] == ref.distinct
    assert_same_as_oracle(kc, ref)


@pytest.mark.parametrize("wmax", [15, 2])
def test_weight_cap(forced, monkeypatch, wmax):
    # multiplicities far above the cap (one k-mer in several entries of full weight and a remainder),
    # counts above 65535 in the result
    monkeypatch.setenv("FASTKMER_DEBUG_FOLD_WMAX", str(wmax))
    kc = count_pinned(skewed(), 28, 10)
    assert kc.stats()["pieces_counted"] >= 4
    assert_folded(kc)
    ref = ref_of("skewed")
    assert max(int(ref.bin_arrays(b)[2].max()) for b in np.nonzero(ref.bin_sizes())[0].tolist()) > 65535
    assert_same_as_oracle(kc, ref)


# What a parameter set reaches, by stats() and the census (debug_tier_stats): with the default cells
# (2^4 per bin of this input) the buckets above the wave tier are 45 of one minimizer cluster each,
# which the split hands whole to the big table -- FASTKMER_DEBUG_MID_PARTS and _SPLIT_RETRY alone meet
# no mid-tier bucket and no split one.  Cells of 8192 keys give the mid tier, the split, the big table
# and the streaming path their buckets, so those hooks are also set together with them.
BIG_CELLS = {"FASTKMER_DEBUG_CELL_TARGET": "8192"}
REACHES = {
    "streaming_all": lambda st, ts: st["oversize_buckets"] >= 1 and ts["nlarge"] == st["oversize_buckets"],
    "big_table": lambda st, ts: st["big_buckets"] >= 1 and ts["nfbG"] > ts["nlarge"] >= 1,
    "mid_whole": lambda st, ts: st["block_buckets"] >= 1 and ts["mid_mode"] == "whole",
    "mid_ranges": lambda st, ts: st["block_buckets"] >= 1 and ts["mid_mode"] == "ranges",
    "mid_1024": lambda st, ts: st["block_buckets"] >= 1 and ts["mid_mode"] is None,
    "split": lambda st, ts: st["split_buckets"] >= 1 and st["sub_buckets"] >= 2 * st["split_buckets"],
}


# (env, use_ht, what the set reaches); the first six are the sets the test began with
TIER_SETS = [
    ({"FASTKMER_DEBUG_LARGE_BUCKETS": "1"}, False, ["streaming_all"]),
    ({"FASTKMER_DEBUG_MID_PARTS": "1"}, False, ["big_table"]),
    ({"FASTKMER_DEBUG_SPLIT_RETRY": "1"}, False, ["big_table"]),
    (BIG_CELLS, False, ["mid_whole", "split", "big_table"]),
    ({**BIG_CELLS, "FASTKMER_DEBUG_FOLD_WMAX": "2"}, False, ["mid_whole", "split", "big_table"]),
    ({}, True, ["big_table"]),
    ({**BIG_CELLS, "FASTKMER_DEBUG_MID_PARTS": "1"}, False, ["mid_ranges", "split", "big_table"]),
    ({**BIG_CELLS, "FASTKMER_DEBUG_MID_PARTS": "0"}, False, ["mid_1024", "split", "big_table"]),
    ({**BIG_CELLS, "FASTKMER_DEBUG_SPLIT_RETRY": "1"}, False, ["mid_whole", "split", "big_table"]),
    ({**BIG_CELLS, "FASTKMER_DEBUG_MID_PARTS": "1"}, True, ["mid_ranges", "split", "big_table"]),
]


@pytest.mark.parametrize("env,use_ht", [(e, h) for e, h, _ in TIER_SETS])
def test_every_tier_sees_weights(forced, monkeypatch, env, use_ht):
    reaches = next(r for e, h, r in TIER_SETS if e == env and h == use_ht)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    kc = count_pinned(skewed(), 28, 10, use_ht=use_ht)
    if "FASTKMER_DEBUG_LARGE_BUCKETS" in env:  # every bucket on the streaming path: no staged pieces, no fold
        assert kc.stats()["pieces_counted"] == 0 and kc.fold_stats()["pieces_folded"] == 0
    else:
        assert_folded(kc)
    st, ts = kc.stats(), kc.debug_tier_stats()
    for what in reaches:
        assert REACHES[what](st, ts), (what, st, ts)
    assert_same_as_oracle(kc, ref_of("skewed"), ordered=not use_ht)


def test_fold_on_and_off_give_the_same_bins(small_pieces, monkeypatch):
    monkeypatch.setenv("FASTKMER_FOLD", "0")
    off = count_pinned(reads_20x(), 28, 10)
    assert off.fold_stats()["pieces_folded"] == 0
    monkeypatch.setenv("FASTKMER_FOLD", "2")
    on = count_pinned(reads_20x(), 28, 10)
    assert_folded(on)
    assert np.array_equal(off.bin_sizes(), on.bin_sizes())
    for b in range(2048):
        k0, c0 = off.get_bin(b)
        k1, c1 = on.get_bin(b)
        assert np.array_equal(k0, k1) and np.array_equal(c0, c1), f"bin {b}"


# ---- the gate

@pytest.mark.parametrize("k,m", [(31, 10), (55, 12)])
def test_keys_without_a_weight_field_are_not_folded(forced, k, m):
    fasta = fk.synth_fasta(30_000, 100, 200_000, seed=0xF0 + k)
    kc = count_pinned(fasta, k, m)
    if k == 55:
        assert kc.stats()["pieces_counted"] == 4
    assert kc.fold_stats() == {"pieces_folded": 0, "entries_in": 0, "entries_out": 0, "sample_ratio": None}
    assert_same_as_oracle(kc, oracle.OracleResult(fasta, k, m, 2048))


def test_auto_gate_declines_reads_without_duplicates(small_pieces, monkeypatch):
    monkeypatch.setenv("FASTKMER_FOLD", "1")
    fasta = fk.synth_fasta(30_000, 100, 300_000_000, seed=0xF02D)  # 0.01x: next to no k-mer twice
    kc = count_pinned(fasta, 28, 10)
    fs = kc.fold_stats()
    assert kc.stats()["pieces_counted"] == 4
    assert fs["pieces_folded"] == 0 and fs["sample_ratio"] is not None and fs["sample_ratio"] > 0.95, fs
    assert_same_as_oracle(kc, oracle.OracleResult(fasta, 28, 10, 2048))


def test_auto_gate_folds_the_20x_reads(small_pieces, monkeypatch):
    monkeypatch.setenv("FASTKMER_FOLD", "1")
    kc = count_pinned(reads_20x(), 28, 10)
    fs = assert_folded(kc)
    assert fs["sample_ratio"] is not None and fs["sample_ratio"] < 0.6, fs
    assert_same_as_oracle(kc, ref_of("reads_20x"))


# ---- odd pieces

def test_fold_with_a_piece_without_kmers(forced):
    a = fk.synth_fasta(8_000, 100, 300_000, seed=0xA7)
    nn = b"".join(b">n%d\n" % i + b"N" * 100 + b"\n" for i in range(20_000))
    b = fk.synth_fasta(8_000, 100, 300_000, seed=0xA8, first_read=8_000)
    fasta = a + nn + b
    kc = count_pinned(fasta, 28, 10)
    assert kc.stats()["pieces_counted"] >= 2
    assert_folded(kc)
    assert_same_as_oracle(kc, oracle.OracleResult(fasta, 28, 10, 2048))


def test_fold_then_fallback_counts_the_whole_input(forced):
    # a 40 KB line after several pieces were staged and folded: the pieces are dropped, the whole
    # input is counted by the two-kernel path
    fasta = fk.synth_fasta(30_000, 100, 600_000, seed=0xA4)
    cut = len(fasta) * 3 // 4 // 114 * 114
    fasta = fasta[:cut] + b">" + b"h" * 40_000 + b"\n" + b"ACGT" * 40 + b"\n" + fasta[cut:]
    kc = count_pinned(fasta, 28, 10)
    st = kc.stats()
    assert st["fused_map"] == 0 and st["pieces_counted"] == 0
    assert kc.fold_stats()["pieces_folded"] == 0  # nothing folded went into the result
    assert_same_as_oracle(kc, oracle.OracleResult(fasta, 28, 10, 2048))
