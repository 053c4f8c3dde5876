"""What a context owns and what a job leaves behind, through the C-ABI (needs a GPU).

fk.live_resources() counts the device allocations, pinned host allocations, events and streams the
library's owner types hold in this process.  Every test here reads it first and asserts on the
difference (other modules' fixtures may hold contexts): whatever a context ran, closing it gives
everything back, and so does a call that fails.  The second half runs two jobs of different input kinds
on one context: the second must count as it does on a fresh context, and as the oracle says.

Inputs are the staged-pieces shape of test_gpu_pieces.py: 40_000 reads of 100 bp (k = 28) or 25_000 of
150 bp (k = 55) under 256 KB segments and 512 KB pieces (4 staged pieces), B = 2048.
"""
import functools
import gc

import numpy as np
import pytest

import fastkmer_amd as fk
import oracle
import staged_util as su
from test_gpu_comm import assert_union_matches_oracle, record_shards, run_local_job
from test_gpu_fastq import fasta_bytes, fastq_bytes, make_records

pytestmark = pytest.mark.gpu

B = 2048
CONFIGS = {28: (10, 100, 40_000), 55: (12, 150, 25_000)}  # k: (m, read length, reads)
MIN_Q = 3  # qualities are uniform over 2..40: one base in 39 is masked, most 55-mers survive
F9 = 9


@pytest.fixture(autouse=True)
def small_pieces(monkeypatch):
    monkeypatch.setenv("FASTKMER_INGEST_SEG", str(256 << 10))
    monkeypatch.setenv("FASTKMER_PIECE_BYTES", str(512 << 10))


def live():
    gc.collect()  # a counter dropped without close() gives its handles back now, not during the test
    return fk.live_resources()


# ---- inputs and what they must count to, computed once

def dense_of_oracle(ref, k):
    """The oracle's result in export_arrays' layout."""
    keys, counts = [], []
    for b in np.nonzero(ref.bin_sizes())[0].tolist():
        hi, lo, cnt = ref.bin_arrays(b)
        keys.append(lo if k <= 32 else np.stack([hi, lo], axis=1).reshape(-1))
        counts.append(cnt)
    return (np.concatenate(keys).astype(np.uint64), np.concatenate(counts).astype(np.uint32),
            ref.bin_sizes().astype(np.uint64), ref.total_kmers, ref.distinct)


def dense_of_pieces(ref, k):
    keys = np.concatenate([su.as_kmers(ref[b][0], k).reshape(-1) for b in range(B)]).astype(np.uint64)
    counts = np.concatenate([ref[b][1] for b in range(B)])
    sizes = np.array([len(ref[b][1]) for b in range(B)], dtype=np.uint64)
    return keys, counts.astype(np.uint32), sizes, int(counts.sum()), int(sizes.sum())


@functools.lru_cache(maxsize=None)
def fasta_of(k):
    m, read_len, reads = CONFIGS[k]
    return fk.synth_fasta(reads, read_len, 1_000_000, seed=0xC0 + k)


@functools.lru_cache(maxsize=None)
def fasta_ref(k):
    return dense_of_oracle(oracle.OracleResult(fasta_of(k), k, CONFIGS[k][0], B), k)


@functools.lru_cache(maxsize=None)
def fastq_case(k):
    """(FASTQ bytes, what they count to under min_quality = MIN_Q): the first 3000 reads of fasta_of(k)."""
    lines = fasta_of(k).split(b"\n")
    records = make_records([lines[i] for i in range(1, 6000, 2)], seed=k)
    ref = oracle.OracleResult(fasta_bytes(records, MIN_Q), k, CONFIGS[k][0], B)
    return fastq_bytes(records), dense_of_oracle(ref, k)


@functools.lru_cache(maxsize=None)
def pieces_case(k):
    """staged_util's smallest two-piece layout: two cells of two bins dealt over two pieces."""
    rng = np.random.default_rng(k)
    m = CONFIGS[k][0]
    cells = [su.one_cell(rng, k, F9, 8, 64, 40, m=m, B=B, bn=0), su.one_cell(rng, k, F9, 16, 100, 60, m=m, B=B, bn=3)]
    pieces = su.deal(rng, cells, 2, k, modes=("random",))
    keys, counts = su.layout(pieces, k, F9, B, rng)
    return keys, counts, dense_of_pieces(su.reference(pieces, k, B), k)


@functools.lru_cache(maxsize=None)
def pinned_of(k):
    import torch
    fasta = fasta_of(k)
    host = torch.empty(len(fasta), dtype=torch.uint8).pin_memory()
    host.numpy()[:] = np.frombuffer(fasta, dtype=np.uint8)
    return host


@functools.lru_cache(maxsize=None)
def device_of(k):
    return pinned_of(k).cuda()


def assert_counted(kc, want, what=""):
    keys, counts, sizes, total, distinct = want
    st = kc.stats()
    assert (st["kmers"], st["distinct"]) == (total, distinct), what
    gk, gc_, gs = kc.export_arrays()
    assert np.array_equal(gs.astype(np.uint64), sizes), what
    assert np.array_equal(gk, keys) and np.array_equal(gc_, counts), what


# ---- the kinds of job; each returns what the context must hold afterwards

def job_pinned(kc):
    kc.set_input_format("fasta")
    kc.ingest_ptr(pinned_of(kc.k).data_ptr(), len(fasta_of(kc.k)))
    kc.finish()
    assert kc.stats()["pieces_counted"] == 4
    return fasta_ref(kc.k)


def job_pageable(kc):
    kc.set_input_format("fasta")
    kc.ingest(fasta_of(kc.k))
    kc.finish()
    return fasta_ref(kc.k)


def job_device(kc):
    kc.set_input_format("fasta")
    kc.ingest_device(device_of(kc.k).data_ptr(), len(fasta_of(kc.k)))
    kc.finish()
    return fasta_ref(kc.k)


def job_fastq(kc):
    data, want = fastq_case(kc.k)
    kc.set_input_format("fastq", MIN_Q)
    kc.ingest(data)
    kc.finish()
    return want


def job_pieces(kc):
    keys, counts, want = pieces_case(kc.k)
    kc.debug_count_pieces(F9, keys, counts)
    assert kc.stats()["pieces_counted"] == 2
    return want


JOBS = {"pinned": job_pinned, "pageable": job_pageable, "device": job_device, "fastq": job_fastq, "pieces": job_pieces}


# ---- 1. create, run, close: every counter returns to where it started

def use_views(kc, tmp_path):
    """Every call that fills ViewBufs or a temporary of its own: bins, lookups, spectrum, read profiles,
    the comparison with a second context, bin files, save and load."""
    fasta = fasta_of(kc.k)
    b = int(np.argmax(kc.bin_sizes()))
    keys, counts = kc.get_bin(b)
    kw = 1 if kc.k <= 32 else 2
    assert np.array_equal(kc.query(keys[:64 * kw]), counts[:64])
    assert int(kc.spectrum(16).sum()) == kc.stats()["distinct"]
    bases, offsets = fk.reads_csr(fasta[:50 * (CONFIGS[kc.k][1] + 14)])
    assert kc.read_counts(bases, offsets).max() >= 1
    with fk.KmerCounter(kc.k, kc.m, 3, B) as other:
        other.ingest(fasta[:len(fasta) // 4])
        other.finish()
        assert int(kc.compare(other, 8, 8).sum()) >= kc.stats()["distinct"]
    kc.write_bins(str(tmp_path))
    kc.save(str(tmp_path / "r.fkdb"))
    with fk.KmerCounter.load(str(tmp_path / "r.fkdb")) as back:
        assert back.stats()["distinct"] == kc.stats()["distinct"]


@pytest.mark.parametrize("job", ["pinned", "pinned_fold2", "pageable", "fastq", "device_k55", "use_ht"])
def test_close_returns_every_resource(monkeypatch, tmp_path, job):
    before = live()
    k = 55 if job == "device_k55" else 28
    if job == "pinned_fold2":
        monkeypatch.setenv("FASTKMER_FOLD", "2")
    kc = fk.KmerCounter(k, CONFIGS[k][0], 3, B, use_ht=job == "use_ht")
    held = live()
    assert held[0] == before[0] and held[2] > before[2] and held[3] >= before[3] + 4  # events and streams, no memory yet
    if job == "use_ht":
        kc.ingest(fasta_of(k))
        kc.finish()
        want = fasta_ref(k)
        assert (kc.stats()["kmers"], kc.stats()["distinct"]) == want[3:]
    else:
        name = job.split("_")[0]
        assert_counted(kc, JOBS[name](kc), job)
        if job == "pinned_fold2":
            assert kc.fold_stats()["pieces_folded"] >= 1
    if job == "pinned":
        use_views(kc, tmp_path)
    assert live()[0] > before[0]
    kc.close()
    assert live() == before


# ---- 2. two in-process ranks

def test_two_ranks_close_returns_every_resource():
    before = live()
    k, m = 28, 10
    ctxs = run_local_job(record_shards(fasta_of(k), 2), k, m, B=B, feed="pinned")
    assert live()[3] > before[3]
    assert ctxs[0].stats()["kmers"] + ctxs[1].stats()["kmers"] == fasta_ref(k)[3]
    assert_union_matches_oracle(ctxs, oracle.OracleResult(fasta_of(k), k, m, B))
    for c in ctxs:
        c.close()
    assert live() == before  # (a communicator's own handles are not counted)


# ---- 3. calls that fail give back what they took

def test_create_on_a_missing_device():
    import torch
    before = live()
    with pytest.raises(fk.FastKmerError) as e:
        fk.KmerCounter(28, 10, 3, B, device=torch.cuda.device_count())
    assert fk.ERRORS[e.value.code] == "FK_E_DEVICE"
    assert live() == before


def test_malformed_fastq_then_a_good_job():
    before = live()
    data, want = fastq_case(28)
    lines = data.split(b"\n")
    del lines[4 * 1000 + 2]  # record 1000 loses its '+' line
    with fk.KmerCounter(28, 10, 3, B, input_format="fastq", min_quality=MIN_Q) as kc:
        kc.ingest(b"\n".join(lines))
        with pytest.raises(fk.FastKmerError) as e:
            kc.finish()
        assert fk.ERRORS[e.value.code] == "FK_E_INVALID"
        assert kc.fastq_info()["first_malformed"] == 1000
        kc.ingest(data)
        kc.finish()
        assert_counted(kc, want)
    assert live() == before


# ---- 4. two jobs on one context: the second counts as on a fresh one

@functools.lru_cache(maxsize=None)
def fresh(k, kind):
    """What a job of this kind leaves on a fresh context; checked against the oracle."""
    with fk.KmerCounter(k, CONFIGS[k][0], 3, B) as kc:
        want = JOBS[kind](kc)
        assert_counted(kc, want, f"fresh {kind}")
        st = kc.stats()
        return kc.export_arrays(), st["kmers"], st["distinct"]


@pytest.mark.parametrize("k", [28, 55])
@pytest.mark.parametrize("second", list(JOBS))
@pytest.mark.parametrize("first", list(JOBS))
def test_second_job_counts_as_on_a_fresh_context(first, second, k):
    before = live()
    (fkeys, fcounts, fsizes), fkmers, fdistinct = fresh(k, second)
    during = live()
    with fk.KmerCounter(k, CONFIGS[k][0], 3, B) as kc:
        assert_counted(kc, JOBS[first](kc), f"{first} first")
        want = JOBS[second](kc)
        st = kc.stats()
        assert (st["kmers"], st["distinct"]) == (fkmers, fdistinct)
        gk, gc_, gs = kc.export_arrays()
        assert np.array_equal(gs, fsizes) and np.array_equal(gk, fkeys) and np.array_equal(gc_, fcounts)
        assert_counted(kc, want, f"{second} after {first}")
    assert during == before and live() == before
