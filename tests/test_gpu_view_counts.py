"""The views over imported results whose every key and count the test chose (needs a GPU).

views_util.Chosen: about 6000 canonical k-mers binned by the oracle, counts dealt from a palette of 37 values (all
ten digit widths, the edges of the 64-entry tile, of the 1024-entry LDS spectrum and of 16 bits, 2^31 - 1, 2^31,
2^32 - 2, 2^32 - 1) as results A and B holding all 37 x 37 pairs; loaded with import_arrays under the default plan
and with many buckets a bin.  Counts of this size never come out of a small job: they reach the ten-digit text,
the top bits of the radix select, sums above 2^32, the comparison's clamp of counts >= 2^31 and the range kernels'
unsigned compares.  Everything is exact and comes from numpy or plain Python."""
import numpy as np
import pytest

import fastkmer_amd as fk
import views_util as vu
from query_util import pack, revcomp
from test_gpu_compare import check_joined_bin, check_matrix
from test_gpu_reads import check_batch, expected_stats
from test_gpu_spectrum import _files as files

pytestmark = pytest.mark.gpu

MAX = fk.MAX_COUNT
PLANS = ["default", "bucket64"]


def flat(t, k, nbins):
    """import_arrays' arguments of a table."""
    return pack(t.hi, t.lo, k), t.count, np.bincount(t.bin, minlength=nbins).astype(np.uint64)


@pytest.fixture(scope="module")
def loaded():
    """loaded(config, plan, monkeypatch) -> (Chosen, A, B): the two results imported once per configuration and plan."""
    cache = {}

    def get(cfg, plan, monkeypatch):
        if (cfg, plan) not in cache:
            if plan == "bucket64":
                monkeypatch.setenv("FASTKMER_DEBUG_IMPORT_BUCKET", "64")
            c = vu.chosen(*cfg)
            kcs = []
            for t in (c.a, c.b):
                kc = fk.KmerCounter(c.k, c.m, 3, c.B)
                kc.import_arrays(*flat(t, c.k, c.nbins))
                kcs.append(kc)
            if plan == "bucket64":
                assert kcs[0].stats()["buckets"] > len(c.a) // 64, "many buckets a bin"
            cache[cfg, plan] = (c, kcs[0], kcs[1])
        return cache[cfg, plan]

    yield get
    for _, ka, kb in cache.values():
        ka.close()
        kb.close()


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("cfg", vu.VIEW_CONFIGS)
def test_text_of_every_digit_width(loaded, monkeypatch, tmp_path, cfg, plan):
    c, ka, _ = loaded(cfg, plan, monkeypatch)
    for i, (lo, hi) in enumerate(((1, MAX), (10 ** 9, MAX), (2 ** 31, 2 ** 31))):
        d = tmp_path / f"r{i}"
        ka.write_bins(str(d), min_count=lo, max_count=None if hi == MAX else hi)
        got, want = files(d), vu.table_texts(c.a, c.k, lo, hi)
        assert sorted(got) == sorted(want) and len(want) > 0
        bad = [f for f in want if got[f] != want[f]]
        assert not bad, f"[{lo}, {hi}]: {len(bad)} files differ, e.g. {bad[0]}: {got[bad[0]][-80:]!r} != {want[bad[0]][-80:]!r}"
    widths = {len(ln.split(b"\t")[1]) for t in files(tmp_path / "r0").values() for ln in t[:-3].splitlines()}
    assert widths == set(range(1, 11))


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("cfg", vu.VIEW_CONFIGS)
def test_ranges_inclusive_at_both_ends(loaded, monkeypatch, cfg, plan):
    c, ka, _ = loaded(cfg, plan, monkeypatch)
    some = [0, 5, c.nbins - 1]
    for lo, hi in [(p, p) for p in vu.PALETTE] + vu.RANGE_PAIRS:
        want = vu.range_sizes(c.a, c.nbins, lo, hi)
        got = ka.bin_sizes(min_count=lo, max_count=hi)
        assert np.array_equal(got, want), f"[{lo}, {hi}]: bins {np.nonzero(got != want)[0][:5]} differ"
        assert want.sum() > 0
        for b in some if lo == hi else range(0, c.nbins, 7):
            keys, counts = ka.get_bin(b, min_count=lo, max_count=hi)
            wk, wc = vu.range_bin(c.a, c.k, b, lo, hi)
            assert np.array_equal(keys, wk) and np.array_equal(counts, wc), f"bin {b} [{lo}, {hi}]"


def check_spectra(kc, t):
    for n in vu.SPECTRA:
        want, want_tail = vu.spectrum(t.count, n)
        got, tail = kc.spectrum(n, return_tail=True)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"n={n}: entries {bad[:5]} are {got[bad[:5]]}, the model has {want[bad[:5]]}"
        assert tail == want_tail and tail > 2 ** 32, f"n={n}: tail k-mers {tail} != {want_tail}"
        assert np.array_equal(kc.spectrum(n), want)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("cfg", vu.VIEW_CONFIGS)
def test_spectrum_with_a_tail_above_2_to_32(loaded, monkeypatch, cfg, plan):
    c, ka, kb = loaded(cfg, plan, monkeypatch)
    check_spectra(ka, c.a)
    check_spectra(kb, c.b)
    # the kernel of results of 2^32 k-mers and more (64-bit LDS entries): a context reads the hook when it is created
    monkeypatch.setenv("FASTKMER_DEBUG_SPECTRUM_WIDE", "1")
    if plan == "bucket64":
        monkeypatch.setenv("FASTKMER_DEBUG_IMPORT_BUCKET", "64")
    with fk.KmerCounter(c.k, c.m, 3, c.B) as wide:
        wide.import_arrays(*flat(c.a, c.k, c.nbins))
        check_spectra(wide, c.a)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("cfg", vu.VIEW_CONFIGS)
def test_lookups_and_profiles_of_large_counts(loaded, monkeypatch, cfg, plan):
    c, ka, _ = loaded(cfg, plan, monkeypatch)
    k, t = c.k, c.a
    assert np.array_equal(ka.query(pack(t.hi, t.lo, k)), t.count)
    assert np.array_equal(ka.query(pack(*revcomp(t.hi, t.lo, k), k)), t.count)
    only_b = t.find(c.b.hi, c.b.lo, k) < 0
    assert only_b.sum() > 500 and not ka.query(pack(c.b.hi[only_b], c.b.lo[only_b], k)).any()
    bases, offsets = c.profile_reads()
    want_c, want_v = check_batch(ka, t, bases, offsets, rng=(2 ** 31, None))
    model_c, model_v = vu.window_counts(t, bases, offsets, k)
    assert np.array_equal(want_c, model_c) and np.array_equal(want_v, model_v)
    st = expected_stats(model_c, model_v, offsets, 2 ** 31)  # the model's, which check_batch held read_stats against
    assert (st["sum"] > 2 ** 32).any() and ((st["min"] < st["median"]) & (st["median"] < st["max"])).any()
    assert (st["hits"] > 0).any() and (st["hits"] < st["windows"]).any() and (st["median"] >= 2 ** 31).any()


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("cfg", vu.VIEW_CONFIGS)
def test_comparison_of_all_pairs_of_counts(loaded, monkeypatch, cfg, plan):
    c, ka, kb = loaded(cfg, plan, monkeypatch)
    p = c.pair
    for rows, cols in vu.SHAPES:
        M = check_matrix(ka, kb, p, rows, cols)  # ... and the transposed call
        assert int(M.sum()) == len(p.ca) and M[rows - 1, cols - 1] > 0
    for side, (x, y) in enumerate(((ka, kb), (kb, ka))):
        for rg in vu.JOINS:
            want = p.sizes(side, rg)
            assert np.array_equal(x.bin_sizes_joined(y, *rg), want), (side, rg)
            assert want.sum() > 0
            for b in np.nonzero(want)[0][[0, -1]].tolist() + [5]:
                assert check_joined_bin(x, y, p, side, b, rg) == want[b]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("cfg", vu.VIEW_CONFIGS)
def test_store_keeps_keys_and_counts(loaded, monkeypatch, tmp_path, cfg, plan):
    c, ka, _ = loaded(cfg, plan, monkeypatch)
    want = flat(c.a, c.k, c.nbins)
    total = sum(int(x) for x in c.a.count)
    assert total > 2 ** 32 and ka.stats()["kmers"] == total and ka.stats()["distinct"] == len(c.a)
    assert all(np.array_equal(x, y) for x, y in zip(ka.export_arrays(), want))
    p1, p2 = str(tmp_path / "one.fkdb"), str(tmp_path / "two.fkdb")
    ka.save(p1)
    ka.save(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    info = fk.db_info(p1)
    assert info["kmers"] == total and info["distinct"] == len(c.a)
    with fk.KmerCounter.load(p1) as copy:
        assert all(np.array_equal(x, y) for x, y in zip(copy.export_arrays(), want))
        assert copy.stats()["kmers"] == total
        assert np.array_equal(copy.query(want[0]), c.a.count)
