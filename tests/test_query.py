"""Host side of the lookups (no GPU): fk_kmer_bin gives every k-mer of every oracle bin that bin, on
either strand -- the bin is a pure function of the k-mer, which is what lets fk_query find a k-mer
without its read -- and encode_keys inverts decode_keys."""
import os

import numpy as np
import pytest

import fastkmer_amd as fk
import oracle
from conftest import GOLDEN, golden_cases
from query_util import CONFIGS, OracleTable, U64, kmer_bins, pack, revcomp


@pytest.fixture(scope="module", autouse=True)
def built():
    from fastkmer_amd import build
    build.build()


def _inputs():
    out = []
    for name, case in sorted(golden_cases().items()):
        with open(os.path.join(GOLDEN, name + ".fa"), "rb") as f:
            out.append((name, f.read(), case.get("sequence_type", 0)))
    for seed in (11, 12):
        out.append((f"synth{seed}", fk.synth_fasta(2000, 100, 100_000, seed=seed), 0))
    return out


INPUTS = _inputs()


@pytest.mark.parametrize("k,m,B", CONFIGS)
@pytest.mark.parametrize("name", [n for n, _, _ in INPUTS])
def test_kmer_bin_is_the_oracle_bin_on_both_strands(name, k, m, B):
    data, seq_type = next((d, s) for n, d, s in INPUTS if n == name)
    res = oracle.OracleResult(data, k, m, B, seq_type)
    tab = OracleTable(res, res.nbins)
    assert len(tab) == res.distinct
    assert res.nbins == fk.clamped_bins(m, B)
    got = kmer_bins(pack(tab.hi, tab.lo, k), k, m, B)
    assert np.array_equal(got, tab.bin)
    rh, rl = revcomp(tab.hi, tab.lo, k)
    got = kmer_bins(pack(rh, rl, k), k, m, B)
    assert np.array_equal(got, tab.bin)
    # the Python wrapper: a key, its pair form and its string
    for i in range(0, len(tab), max(1, len(tab) // 5)):
        key = pack(tab.hi[i:i + 1], tab.lo[i:i + 1], k)
        assert fk.kmer_bin(key, k, m, B) == tab.bin[i]
        assert fk.kmer_bin(fk.decode_keys(key, k)[0], k, m, B) == tab.bin[i]


def test_kmer_bin_of_forbidden_mmers_uses_signature_4_pow_m():
    # (AATT)*: every 10-mer holds "AA", and so does its reverse complement ("TT" forward)
    k, m, B = 28, 10, 2048
    kmer = "AATT" * 7
    assert all(oracle.norm(int(fk.encode_keys([kmer[i:i + m]], m)[0]), m) == 4 ** m for i in range(k - m + 1))
    want = oracle.hash_to_bucket(4 ** m, B)
    assert fk.kmer_bin(kmer, k, m, B) == want
    res = oracle.OracleResult(b">r\n" + kmer.encode() + b"\n", k, m, B)
    assert res.distinct == 1 and res.bin_size(want) == 1
    # poly-A is not such a k-mer: its reverse strand's m-mers (poly-T) are allowed
    assert fk.kmer_bin("A" * k, k, m, B) == oracle.hash_to_bucket(4 ** m - 1, B) == fk.kmer_bin("T" * k, k, m, B)


@pytest.mark.parametrize("k", [5, 28, 32, 33, 55, 64])
def test_encode_keys_inverts_decode_keys(k):
    rng = np.random.default_rng(k)
    kw = 2 if k > 32 else 1
    x = rng.integers(0, 2 ** 64, size=200 * kw, dtype=U64)
    if k < 32:
        x &= U64((1 << (2 * k)) - 1)
    elif 32 < k < 64:
        x[0::2] &= U64((1 << (2 * k - 64)) - 1)
    strs = fk.decode_keys(x, k)
    assert all(len(s) == k and set(s) <= set("ACGT") for s in strs)
    assert np.array_equal(fk.encode_keys(strs, k), x)
    assert fk.encode_keys([], k).size == 0


@pytest.mark.parametrize("bad", [["ACGN"], ["acgt"], ["ACG"], ["ACGTA"], ["ACGT", "AC T"]])
def test_encode_keys_refuses_bad_input(bad):
    with pytest.raises(ValueError):
        fk.encode_keys(bad, 4)


@pytest.mark.parametrize("k,m,B", [(28, 10, 2048), (55, 12, 8192)])
def test_key_with_a_bit_above_2k_is_invalid(k, m, B):
    top = 2 * k  # the first bit that is no base of the k-mer
    key = np.array([1 << top], dtype=U64) if k <= 32 else np.array([1 << (top - 64), 0], dtype=U64)
    with pytest.raises(fk.FastKmerError) as e:
        fk.kmer_bin(key, k, m, B)
    assert e.value.code == -1
    key[0] = (1 << 63)
    with pytest.raises(fk.FastKmerError) as e:
        fk.kmer_bin(key, k, m, B)
    assert e.value.code == -1
    # the largest k-mer itself is fine
    assert 0 <= fk.kmer_bin("T" * k, k, m, B) < fk.clamped_bins(m, B)


def test_kmer_bin_applies_the_configuration_checks():
    for k, m, B in [(28, 16, 2048), (9, 10, 2048), (65, 10, 2048), (28, 10, 0)]:
        with pytest.raises(fk.FastKmerError) as e:
            fk.kmer_bin(np.zeros(2 if k > 32 else 1, dtype=U64), k, m, B)
        assert e.value.code == -1
