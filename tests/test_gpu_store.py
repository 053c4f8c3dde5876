"""Export, import and the database file of a counted result (fk_export*, fk_import*, fk_save, fk_load)
on the GPU, through the C-ABI.

A loaded or imported context must answer every result call exactly as the context the result was counted
in: bins, sizes, spectrum, lookups on both strands, read profiles, the comparison (diagonal both ways), and
a following job.  The import's bucket tables are driven to their shapes with FASTKMER_DEBUG_IMPORT_BUCKET
and FASTKMER_DEBUG_CELL_TARGET over arrays built in numpy from random canonical keys binned by fk_query's
own `bins` output; its verify pass is fed one defect at a time."""
import os
import subprocess

import numpy as np
import pytest

import fastkmer_amd as fk
from conftest import GOLDEN
from test_gpu_comm import record_shards, run_local_job

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_IO = -1, -2, -5
U32_MAX = 0xFFFFFFFF
DB = os.path.join(GOLDEN, "store_k21.fkdb")


def fasta_small(seed=7):
    return fk.synth_fasta(2000, 100, 40_000, seed=seed)


# ---- numpy reverse complement of keys in get_bin's layout (rows of one word, or (hi, lo))
def _rev_pairs(x):
    """the 32 two-bit groups of every uint64 in reverse order"""
    x = ((x >> np.uint64(2)) & np.uint64(0x3333333333333333)) | ((x & np.uint64(0x3333333333333333)) << np.uint64(2))
    x = ((x >> np.uint64(4)) & np.uint64(0x0F0F0F0F0F0F0F0F)) | ((x & np.uint64(0x0F0F0F0F0F0F0F0F)) << np.uint64(4))
    return x.byteswap()


def revcomp(keys, k):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if k <= 32:
        return _rev_pairs(~keys.reshape(-1)) >> np.uint64(64 - 2 * k)
    hi, lo = keys.reshape(-1, 2)[:, 0], keys.reshape(-1, 2)[:, 1]
    rhi, rlo = _rev_pairs(~lo), _rev_pairs(~hi)  # the 128-bit reversal, then >> (128 - 2k)
    s = np.uint64(128 - 2 * k)
    return np.stack([rhi >> s, (rlo >> s) | (rhi << (np.uint64(64) - s))], axis=1).reshape(-1)


def random_keys(rng, k, n):
    """n random 2k-bit keys in get_bin's layout"""
    lo = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    if k <= 32:
        return lo >> np.uint64(64 - 2 * k)
    hi = rng.integers(0, 1 << (2 * k - 64), size=n, dtype=np.uint64)
    return np.stack([hi, lo], axis=1).reshape(-1)


def canonical(keys, k):
    kw = 2 if k > 32 else 1
    f, r = keys.reshape(-1, kw), revcomp(keys, k).reshape(-1, kw)
    less = (r[:, 0] < f[:, 0]) if kw == 1 else ((r[:, 0] < f[:, 0]) | ((r[:, 0] == f[:, 0]) & (r[:, 1] < f[:, 1])))
    return np.where(less[:, None], r, f)


def binned_random(kc, k, n, rng):
    """{bin: sorted unique canonical keys (rows)} of n random k-mers, binned by fk_query's bins output"""
    rows = np.unique(canonical(random_keys(rng, k, n), k), axis=0)  # lexicographic rows: ascending keys
    _, bins = kc.query(rows.reshape(-1), return_bins=True)
    return {int(b): rows[bins == b] for b in np.unique(bins)}


def flat(bins, counts):
    """(keys, counts, bin_sizes) of {bin: rows} / {bin: counts} in ascending bin order"""
    order = sorted(bins)
    nb = 64
    sizes = np.zeros(nb, dtype=np.uint64)
    for b in order:
        sizes[b] = len(bins[b])
    keys = np.concatenate([bins[b].reshape(-1) for b in order]) if order else np.zeros(0, np.uint64)
    cnts = np.concatenate([counts[b] for b in order]) if order else np.zeros(0, np.uint32)
    return keys, cnts.astype(np.uint32), sizes


def assert_same_answers(a, b, fasta, k, rng):
    """b answers every result call as a does"""
    sizes = a.bin_sizes()
    assert np.array_equal(sizes, b.bin_sizes())
    stored = []
    for bin_ in np.nonzero(sizes)[0].tolist():
        ka, ca = a.get_bin(bin_)
        kb, cb = b.get_bin(bin_)
        assert np.array_equal(ka, kb) and np.array_equal(ca, cb), f"bin {bin_}"
        stored.append(ka)
    assert np.array_equal(a.spectrum(64), b.spectrum(64))
    stored = np.concatenate(stored) if stored else np.zeros(0, np.uint64)
    probe = np.concatenate([stored, revcomp(stored, k), random_keys(rng, k, 2000)])
    ca, ba = a.query(probe, return_bins=True)
    cb, bb = b.query(probe, return_bins=True)
    assert np.array_equal(ca, cb) and np.array_equal(ba, bb)
    n = stored.size // (2 if k > 32 else 1)
    assert np.all(ca[:2 * n] > 0) and np.array_equal(ca[:n], ca[n:2 * n])
    if a.n_ranks == 1:
        assert np.array_equal(a.read_stats(fasta), b.read_stats(fasta))
    for x, y in ((a, b), (b, a)):
        m = x.compare(y, 32, 32)
        assert m.sum() == np.trace(m) == sizes.sum(), "the comparison is not diagonal"
    sa, sb = a.stats(), b.stats()
    assert sb["distinct"] == sa["distinct"] == sizes.sum()


@pytest.fixture(scope="module")
def refs():
    """One counted context per k, shared and left unchanged."""
    made = {}

    def get(k):
        if k not in made:
            kc = fk.KmerCounter(k, 5, 3, 64)
            kc.ingest(fasta_small())
            kc.finish()
            made[k] = kc
        return made[k]

    yield get
    for kc in made.values():
        kc.close()


# ---- 1. round trip through a file
@pytest.mark.parametrize("k", [21, 28, 31, 32, 33, 55, 63])
def test_round_trip(refs, tmp_path, k):
    a = refs(k)
    path = str(tmp_path / "a.fkdb")
    a.save(path)
    info = fk.db_info(path)
    assert (info["k"], info["m"], info["bins"], info["key_words"]) == (k, 5, 64, 2 if k > 32 else 1)
    assert info["distinct"] == a.stats()["distinct"] and info["kmers"] == a.stats()["kmers"]
    assert not os.path.exists(path + ".tmp")
    rng = np.random.default_rng(k)
    with fk.KmerCounter.load(path) as b:
        assert b.stats()["kmers"] == info["kmers"] and b.stats()["ms_count"] == 0
        assert_same_answers(a, b, fasta_small(), k, rng)
        # a fresh job on the loaded context counts correctly
        other = fasta_small(seed=11)
        b.ingest(other)
        b.finish()
        with fk.KmerCounter(k, 5, 3, 64) as c:
            c.ingest(other)
            c.finish()
            assert_same_answers(c, b, other, k, rng)


def test_export_import_arrays_round_trip(refs):
    a = refs(28)
    keys, counts, sizes = a.export_arrays()
    cut = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for b in np.nonzero(sizes)[0].tolist():  # fk_bin_sizes gives the cut points
        kb, cb = a.get_bin(b)
        assert np.array_equal(keys[cut[b]:cut[b + 1]], kb) and np.array_equal(counts[cut[b]:cut[b + 1]], cb)
    with fk.KmerCounter(28, 5, 3, 64) as b:
        b.import_arrays(keys, counts, sizes)
        assert_same_answers(a, b, fasta_small(), 28, np.random.default_rng(1))
        st = b.stats()
        assert st["kmers"] == int(counts.sum(dtype=np.uint64)) and st["buckets"] > 0 and st["fine_bits"] >= 1
        assert st["ms_total"] == 0 and st["superkmers"] == 0 and st["fasta_bytes"] == 0
    with fk.KmerCounter(28, 5, 3, 64) as c:
        c.import_bins({b: a.get_bin(b) for b in np.nonzero(sizes)[0].tolist()})
        assert np.array_equal(c.export_arrays()[0], keys)


def test_export_import_device_pointers(refs):
    import torch
    a = refs(55)
    n = a.stats()["distinct"]
    dk = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    dc = torch.zeros(n, dtype=torch.int32, device="cuda")
    with pytest.raises(fk.FastKmerError) as e:
        a.export_ptr(dk.data_ptr(), dc.data_ptr(), n - 1)
    assert e.value.code == -6
    assert a.export_ptr(dk.data_ptr(), dc.data_ptr(), n) == n
    torch.cuda.synchronize()
    keys, counts, sizes = a.export_arrays()
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), keys) and np.array_equal(dc.cpu().numpy().view(np.uint32), counts)
    with fk.KmerCounter(55, 5, 3, 64) as b:
        b.import_ptr(dk.data_ptr(), dc.data_ptr(), sizes)
        dk.zero_()  # the arrays were copied
        torch.cuda.synchronize()
        assert_same_answers(a, b, fasta_small(), 55, np.random.default_rng(2))


# ---- 2. byte identity with the committed file
def test_save_is_byte_identical_to_the_golden_file(tmp_path):
    with open(os.path.join(GOLDEN, "edge_bytes_k21.fa"), "rb") as f:
        fasta = f.read()
    with open(DB, "rb") as f:
        want = f.read()
    p1, p2 = str(tmp_path / "one.fkdb"), str(tmp_path / "two.fkdb")
    with fk.KmerCounter(21, 7, 2, 64) as kc:
        kc.ingest(fasta)
        kc.finish()
        kc.save(p1)
    assert open(p1, "rb").read() == want
    with fk.KmerCounter.load(DB) as kc:
        kc.save(p2)
    assert open(p2, "rb").read() == want


# ---- 3. the import's bucket shapes
@pytest.mark.parametrize("k,cell_target", [(21, 4), (21, 1_000_000), (31, 64), (55, 4), (55, 1_000_000), (63, 64)])
def test_import_bucket_shapes(refs, monkeypatch, k, cell_target):
    rng = np.random.default_rng(100 * k + cell_target % 97)
    bins = binned_random(refs(k), k, 20_000, rng)
    by_size = sorted(bins, key=lambda b: -len(bins[b]))
    one_cell, single, emptied = by_size[0], by_size[1], by_size[2:6]
    assert len(bins) > 32 and len(bins[one_cell]) > 400
    kw = 2 if k > 32 else 1
    top = bins[one_cell][:, 0] >> np.uint64((2 * k - 1) % 64)  # the key's highest bit: its cell at F = 1
    bins[one_cell] = bins[one_cell][top == 0]  # a bin inside one cell when the cells are coarse: a bucket above the target
    assert len(bins[one_cell]) > 64
    bins[single] = bins[single][:1]            # a bin with one key
    for b in emptied:                          # empty bins between full ones
        del bins[b]
    counts = {b: rng.choice(np.array([1, 1, 2, 77, U32_MAX], dtype=np.uint64), size=len(v)) for b, v in bins.items()}
    counts[single][:] = U32_MAX
    keys, cnts, sizes = flat(bins, counts)
    monkeypatch.setenv("FASTKMER_DEBUG_IMPORT_BUCKET", "64")
    monkeypatch.setenv("FASTKMER_DEBUG_CELL_TARGET", str(cell_target))
    with fk.KmerCounter(k, 5, 3, 64) as kc:
        kc.import_arrays(keys, cnts, sizes)
        st = kc.stats()
        assert st["distinct"] == cnts.size and st["kmers"] == int(cnts.sum(dtype=np.uint64))
        assert (st["fine_bits"] == 1) == (cell_target > 1000)
        assert st["buckets"] > (64 if cell_target > 1000 else cnts.size // 64)  # bins spanning many buckets
        assert np.array_equal(kc.bin_sizes(), sizes)
        for b, rows in bins.items():
            kb, cb = kc.get_bin(b)
            assert np.array_equal(kb, rows.reshape(-1)) and np.array_equal(cb, counts[b].astype(np.uint32)), f"bin {b}"
        # every stored key is found, on both strands; keys of the emptied bins are not
        got, where = kc.query(keys, return_bins=True)
        assert np.array_equal(got, cnts) and np.array_equal(where, np.repeat(np.arange(64), sizes.astype(np.int64)))
        assert np.array_equal(kc.query(revcomp(keys, k)), cnts)
        assert not kc.query(random_keys(rng, k, 3000)).any()
        ek, ec, es = kc.export_arrays()
        assert np.array_equal(ek, keys) and np.array_equal(ec, cnts) and np.array_equal(es, sizes)
        hist, tail = kc.spectrum(4, return_tail=True)
        assert hist.tolist() == [0, int((cnts == 1).sum()), int((cnts == 2).sum()), int((cnts > 2).sum())]
        assert tail == int(cnts[cnts > 2].sum(dtype=np.uint64))
        # an empty result
        kc.import_arrays(np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(64, np.uint64))
        assert kc.stats()["distinct"] == 0 and not kc.bin_sizes().any() and not kc.query(keys[:kw * 10]).any()
        assert kc.export_arrays()[0].size == 0 and not kc.spectrum(8).any()
        # ... and a job after it
        kc.ingest(fasta_small())
        kc.finish()
        assert np.array_equal(kc.bin_sizes(), refs(k).bin_sizes())


def test_empty_result_saves_a_header_with_no_bins(tmp_path):
    path = str(tmp_path / "empty.fkdb")
    with fk.KmerCounter(21, 7, 1, 64) as kc:
        kc.ingest(b"")
        kc.finish()
        kc.save(path)
    info = fk.db_info(path)
    assert info["file_bytes"] == 72 and info["stored_bins"] == 0 and info["distinct"] == info["kmers"] == info["checksum"] == 0
    with fk.KmerCounter.load(path) as kc:
        assert kc.stats()["distinct"] == 0 and not kc.bin_sizes().any()


# ---- 4. what the import refuses
def _defects(A, B, k):
    """(name, change(bins, counts) -> (bin, index), reason) one defect each, in bin A (and bin B)"""
    kw = 2 if k > 32 else 1

    def swap(b, c):
        b[A][[7, 8]] = b[A][[8, 7]]
        return A, 8

    def dup(b, c):
        b[A][8] = b[A][7]
        return A, 8

    def strand(b, c):
        b[A][7] = revcomp(b[A][7], k).reshape(kw)
        return A, 7

    def wrong_bin(b, c):
        b[B] = np.concatenate([b[A][-1:], b[B]])
        c[B] = np.concatenate([c[A][-1:], c[B]])
        b[A], c[A] = b[A][:-1], c[A][:-1]
        return B, 0

    def high_bit(b, c):
        b[A][7, 0] |= np.uint64(1) << np.uint64((2 * k) % 64)
        return A, 7

    def zero(b, c):
        c[A][7] = 0
        return A, 7

    return [("swapped pair", swap, "not ascending"), ("duplicate", dup, "duplicate"), ("non-canonical", strand, "not canonical"),
            ("wrong bin", wrong_bin, "another bin"), ("high bit", high_bit, "above bit 2k - 1"), ("zero count", zero, "count 0")]


@pytest.mark.parametrize("k", [31, 55])
def test_import_refusals(refs, k):
    rng = np.random.default_rng(k)
    good = binned_random(refs(k), k, 6000, rng)
    A, B = sorted(good, key=lambda b: -len(good[b]))[:2]
    assert len(good[A]) > 16 and len(good[B]) > 16
    for name, change, reason in _defects(A, B, k):
        bins = {b: v.copy() for b, v in good.items()}
        counts = {b: np.full(len(v), 3, dtype=np.uint64) for b, v in bins.items()}
        bad_bin, idx = change(bins, counts)
        with fk.KmerCounter(k, 5, 3, 64) as kc:
            kc.import_arrays(*flat(good, {b: np.full(len(v), 3, dtype=np.uint64) for b, v in good.items()}))
            assert kc.bin_sizes().sum() > 0
            with pytest.raises(fk.FastKmerError) as e:
                kc.import_arrays(*flat(bins, counts))
            msg = str(e.value)
            assert e.value.code == E_INVALID and f"bin {bad_bin}, key {idx}:" in msg and reason in msg, (name, msg)
            with pytest.raises(fk.FastKmerError) as e:  # the context is left without a result
                kc.bin_sizes()
            assert e.value.code == E_STATE
            with pytest.raises(fk.FastKmerError) as e:
                kc.query(good[A].reshape(-1))
            assert e.value.code == E_STATE


def test_import_refuses_another_ranks_bin(refs):
    good = binned_random(refs(31), 31, 3000, np.random.default_rng(5))
    counts = {b: np.ones(len(v), dtype=np.uint64) for b, v in good.items()}
    mine = {b: v for b, v in good.items() if b % 2 == 0}
    even, odd, other = min(mine), min(b for b in good if b % 2), max(b for b in good if b % 2)
    with fk.KmerCounter(31, 5, 3, 64, n_ranks=2, rank=0) as kc:
        kc.import_arrays(*flat(mine, counts))  # its own bins: fine
        assert np.array_equal(np.nonzero(kc.bin_sizes())[0], np.array(sorted(mine)))
        assert np.array_equal(kc.query(good[even].reshape(-1)), counts[even]) and not kc.query(good[odd].reshape(-1)).any()
        mine[other] = good[other]
        with pytest.raises(fk.FastKmerError) as e:
            kc.import_arrays(*flat(mine, counts))
        assert e.value.code == E_INVALID and f"bin {other} " in str(e.value) and "rank 1" in str(e.value)
        with pytest.raises(fk.FastKmerError) as e:
            kc.bin_sizes()
        assert e.value.code == E_STATE


def test_import_inside_a_job_is_a_state_error(refs):
    keys, counts, sizes = refs(28).export_arrays()
    with fk.KmerCounter(28, 5, 3, 64) as kc:
        kc.ingest_chunk(fasta_small()[:11400], last=False)
        with pytest.raises(fk.FastKmerError) as e:
            kc.import_arrays(keys, counts, sizes)
        assert e.value.code == E_STATE
        kc.ingest_chunk(fasta_small()[11400:], last=True)
        kc.finish()
        assert np.array_equal(kc.bin_sizes(), sizes)


# ---- 5. corrupt files
def test_corrupt_files_are_refused(refs, tmp_path):
    path = str(tmp_path / "a.fkdb")
    refs(28).save(path)
    raw = open(path, "rb").read()
    info = fk.db_info(path)
    hb = 72 + 16 * info["stored_bins"]
    key_end = hb + 8 * info["distinct"]
    bad = str(tmp_path / "bad.fkdb")
    with fk.KmerCounter(28, 5, 3, 64) as kc:
        for at, bit in ((hb + 8 * 100 + 1, 0x04), (key_end + 4 * 100, 0x10)):  # a key bit, a count bit
            b = bytearray(raw)
            b[at] ^= bit
            open(bad, "wb").write(bytes(b))
            with pytest.raises(fk.FastKmerError) as e:
                kc.load_into(bad)
            assert e.value.code == E_INVALID, str(e.value)
            with pytest.raises(fk.FastKmerError) as e:
                kc.bin_sizes()
            assert e.value.code == E_STATE
        b = bytearray(raw)  # two counts exchanged: every check of the import passes, the checksum does not
        b[key_end:key_end + 4], b[key_end + 4:key_end + 8] = raw[key_end + 4:key_end + 8], raw[key_end:key_end + 4]
        if b != bytearray(raw):
            open(bad, "wb").write(bytes(b))
            with pytest.raises(fk.FastKmerError) as e:
                kc.load_into(bad)
            assert e.value.code == E_INVALID and "checksum" in str(e.value)
        open(bad, "wb").write(raw[:key_end + 40])
        with pytest.raises(fk.FastKmerError) as e:
            kc.load_into(bad)
        assert e.value.code == E_IO and "truncated" in str(e.value)
        kc.load_into(path)  # and the good file still loads
        assert np.array_equal(kc.bin_sizes(), refs(28).bin_sizes())
    with fk.KmerCounter(28, 6, 3, 64) as kc:  # another m: refused by name
        with pytest.raises(fk.FastKmerError) as e:
            kc.load_into(path)
        assert e.value.code == E_INVALID and "m = 5" in str(e.value)
    with fk.KmerCounter(29, 5, 3, 64) as kc:
        with pytest.raises(fk.FastKmerError) as e:
            kc.load_into(path)
        assert e.value.code == E_INVALID and "k = 28" in str(e.value)
    with fk.KmerCounter(28, 5, 3, 32) as kc:
        with pytest.raises(fk.FastKmerError) as e:
            kc.load_into(path)
        assert e.value.code == E_INVALID and "bins = 64" in str(e.value)


# ---- 6. ranks
def test_two_rank_files(tmp_path):
    fasta = fasta_small()
    ctxs = run_local_job(record_shards(fasta, 2), 28, 5, 3, 64)
    paths = [str(tmp_path / f"rank{r}.fkdb") for r in range(2)]
    rng = np.random.default_rng(3)
    try:
        for kc, p in zip(ctxs, paths):
            kc.save(p)
        assert [(fk.db_info(p)["n_ranks"], fk.db_info(p)["rank"]) for p in paths] == [(2, 0), (2, 1)]
        for r in range(2):  # each file into the same rank of a fresh pair
            with fk.KmerCounter.load(paths[r], n_ranks=2, rank=r) as b:
                assert_same_answers(ctxs[r], b, fasta, 28, rng)
        sizes1 = ctxs[1].bin_sizes()
        assert not sizes1[0::2].any() and sizes1[1::2].any()
        with fk.KmerCounter.load(paths[1]) as one:  # rank 1's file into a one-rank context: exactly its bins
            assert one.n_ranks == 1 and np.array_equal(one.bin_sizes(), sizes1)
            for b in np.nonzero(sizes1)[0].tolist():
                assert all(np.array_equal(x, y) for x, y in zip(one.get_bin(b), ctxs[1].get_bin(b)))
            k0 = np.concatenate([ctxs[0].get_bin(b)[0] for b in np.nonzero(ctxs[0].bin_sizes())[0].tolist()])
            k1 = ctxs[1].export_arrays()[0]
            assert not one.query(k0).any() and np.array_equal(one.query(k1), ctxs[1].query(k1))
        with fk.KmerCounter(28, 5, 3, 64, n_ranks=2, rank=0) as zero:  # ... and into rank 0: refused
            with pytest.raises(fk.FastKmerError) as e:
                zero.load_into(paths[1])
            assert e.value.code == E_INVALID and "belongs to rank 1" in str(e.value)
    finally:
        for kc in ctxs:
            kc.close()


# ---- 7. the CLI
def test_cli_save_and_compare_with_a_database(tmp_path):
    fa, fb = tmp_path / "a.fa", tmp_path / "b.fa"
    fa.write_bytes(fasta_small())
    fb.write_bytes(fasta_small(seed=11)[:114 * 1200] + fasta_small()[:114 * 500])
    db = tmp_path / "b.fkdb"
    base = {k: v for k, v in os.environ.items() if not k.startswith("FASTKMER_CLI_")}

    def run(inp, prefix, use_ht=0, **env):
        r = subprocess.run([fk.CLI_PATH, "28", "5", "3", "64", str(use_ht), "0", str(inp), str(tmp_path) + "/", prefix, "0", "0",
                            "0"], capture_output=True, text=True, env=dict(base, **env))
        return r, tmp_path / f"{prefix}k28_m5_x3_b64_s0" / "compare.tsv"

    r, _ = run(fb, "save_", FASTKMER_CLI_SAVE=str(db))
    assert r.returncode == 0 and "Database written" in r.stdout, r.stderr
    assert fk.db_info(str(db))["k"] == 28
    r1, t1 = run(fa, "fasta_", FASTKMER_CLI_COMPARE=str(fb))
    r2, t2 = run(fa, "db_", FASTKMER_CLI_COMPARE=str(db))
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    assert t1.read_bytes() == t2.read_bytes() and len(t1.read_bytes().splitlines()) > 3
    r, _ = run(fb, "ht_", use_ht=1, FASTKMER_CLI_SAVE=str(tmp_path / "ht.fkdb"))
    assert r.returncode == 2 and "FASTKMER_CLI_SAVE needs the sorted count" in r.stderr and "usage" in r.stderr


# ---- 8. use_ht = 1
def test_use_ht_is_refused(refs, tmp_path):
    keys, counts, sizes = refs(21).export_arrays()
    with open(os.path.join(GOLDEN, "edge_bytes_k21.fa"), "rb") as f:
        fasta = f.read()
    with fk.KmerCounter(21, 7, 2, 64, use_ht=True) as kc:
        kc.ingest(fasta)
        kc.finish()
        before = kc.bin_sizes()
        for call in (lambda: kc.save(str(tmp_path / "ht.fkdb")), kc.export_arrays, lambda: kc.load_into(DB),
                     lambda: kc.import_arrays(np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(64, np.uint64))):
            with pytest.raises(fk.FastKmerError) as e:
                call()
            assert e.value.code == E_INVALID and "use_ht" in str(e.value)
        assert np.array_equal(kc.bin_sizes(), before) and not os.path.exists(tmp_path / "ht.fkdb")
