"""bench.py's plain and --full runs and --dump-outputs: a plain run times the headline leg alone,
the other legs need --full, and --dump-outputs writes the last timed step's counts as float64 .npy
files (checked against the CPU oracle on the GPU; the file layout with a stand-in counter here)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("device_resident_value", "device_resident_ms_per_step", "roofline", "configs2_per_gpu", "cpu_baseline")


def _run(args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=timeout)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _keys(halves):
    """sample_keys.npy rows (32-bit halves, most significant first) back to uint64 words."""
    h = halves.astype(np.uint64)
    return (h[:, 0::2] << np.uint64(32)) | h[:, 1::2]


@pytest.mark.parametrize("args", [["--device-leg"], ["--c3-leg", "on"]])
def test_other_legs_need_full(args):
    p = _run(["--gpus", "1", "--steps", "1"] + args)
    assert p.returncode == 2 and "--full" in p.stderr and p.stdout == ""


class _Counter:
    """The results API of KmerCounter over made-up bins, entries in no particular order."""

    def __init__(self, k, n_bins=64, seed=3):
        rng = np.random.default_rng(seed)
        self.k, self.kw = k, 2 if k > 32 else 1
        self.bins = []
        for b in range(n_bins):
            n = int(rng.integers(0, 50))
            keys = rng.integers(0, 1 << 62, (n, self.kw), dtype=np.uint64)
            if self.kw == 2 and n > 1:
                keys[1, 0] = keys[0, 0]  # equal high words: the low word decides the order
            self.bins.append((keys, rng.integers(1, 1 << 31, n, dtype=np.uint32)))

    def bin_sizes(self):
        return np.array([len(c) for _, c in self.bins], dtype=np.uint64)

    def get_bin(self, b):
        return self.bins[b][0].reshape(-1).copy(), self.bins[b][1].copy()

    def stats(self):
        return {"kmers": int(sum(int(c.sum()) for _, c in self.bins)), "distinct": int(self.bin_sizes().sum())}


@pytest.mark.parametrize("k", [28, 55])
def test_dump_outputs_layout(tmp_path, k):
    sys.path.insert(0, ROOT)
    import bench
    kc = _Counter(k)
    bench.dump_outputs(kc, str(tmp_path / "a"))
    bench.dump_outputs(kc, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["bin_sizes", "sample_bins", "sample_counts", "sample_keys", "sample_offsets", "totals"]
    for name in a:
        assert a[name].dtype == np.float64 and np.array_equal(a[name], b[name]), name
    assert np.array_equal(a["bin_sizes"], kc.bin_sizes().astype(np.float64))
    assert a["totals"].tolist() == [kc.stats()["kmers"], kc.stats()["distinct"]]
    bins, off = a["sample_bins"].astype(int).tolist(), a["sample_offsets"].astype(int)
    assert len(bins) == bench.DUMP_SAMPLE_BINS == len(set(bins)) and off[0] == 0
    keys = _keys(a["sample_keys"])
    assert keys.shape == (off[-1], kc.kw) and a["sample_counts"].shape == (off[-1],)
    for i, bn in enumerate(bins):
        got = {tuple(r): c for r, c in zip(keys[off[i]:off[i + 1]].tolist(), a["sample_counts"][off[i]:off[i + 1]])}
        exp = {tuple(r): float(c) for r, c in zip(kc.bins[bn][0].tolist(), kc.bins[bn][1])}
        assert got == exp, bn
        rows = keys[off[i]:off[i + 1]].tolist()
        assert rows == sorted(rows), bn


def test_dump_outputs_stays_under_its_budget(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    kc = _Counter(28)
    order = np.random.default_rng(bench.SEED).permutation(64)[:bench.DUMP_SAMPLE_BINS].tolist()
    sizes = kc.bin_sizes()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", int(sizes[order[0]] + sizes[order[1]]) * 24)
    bench.dump_outputs(kc, str(tmp_path))
    d = _load(tmp_path)
    got = d["sample_bins"].astype(int).tolist()
    assert 2 <= len(got) < len(order) and got == order[:len(got)]  # the seeded order, cut at the budget
    assert d["sample_keys"].nbytes + d["sample_counts"].nbytes <= bench.DUMP_MAX_BYTES


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_counts(tmp_path):
    """A plain run at 5 MB: the line holds the headline figures and none of the --full legs, --steps
    sets the timed steps, and the dumped counts are the oracle's over bench.py's own input."""
    import fastkmer_amd as fk
    import oracle
    nbytes = 5_000_000
    p = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--bytes-per-gpu", str(nbytes),
              "--dump-outputs", str(tmp_path / "out")])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "bases/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    assert line["ms_per_step"] > 0
    n_reads = nbytes // 114
    assert line["value"] == pytest.approx(n_reads * 100 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    ref = oracle.OracleResult(fk.synth_fasta(n_reads, 100, 100_000_000, seed=0x5EED), 28, 10, 2048)
    d = _load(tmp_path / "out")
    assert all(v.dtype == np.float64 for v in d.values())
    assert sum(v.nbytes for v in d.values()) <= 64 << 20
    assert np.array_equal(d["bin_sizes"], ref.bin_sizes().astype(np.float64))
    assert d["totals"].tolist() == [ref.total_kmers, ref.distinct]
    bins, off = d["sample_bins"].astype(int).tolist(), d["sample_offsets"].astype(int)
    assert len(bins) == 8 and off[-1] > 0
    keys = _keys(d["sample_keys"])[:, 0]
    for i, b in enumerate(bins):
        _, rlo, rcnt = ref.bin_arrays(b)
        assert np.array_equal(keys[off[i]:off[i + 1]], rlo) and np.array_equal(d["sample_counts"][off[i]:off[i + 1]], rcnt), b
