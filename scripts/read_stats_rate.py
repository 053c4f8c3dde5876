"""The rate of per-read abundance profiles (fk_read_counts_device, fk_read_stats_device) against the
route a caller had without them: fk_query_sequence over the reads joined by 'N' (one call, the best
that interface allows) and a numpy reduction per read on the host.

A configs[1]-parameter job (k=28 m=10 B=2048) of --reads synthetic 100 bp reads is counted on the
device and those same reads are profiled.  The device forms are timed with device events over
--launches launches after --warmup warm-ups; the host route once, by the host clock.  Both routes must
give the same statistics.  Writes a small report (--out).

The window kernel against k_query_seq, kernel time for the same bases, comes from a kernel trace made
in a run of its own (tracing slows the host), whose statistics file is then handed to the report:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- \\
      python scripts/read_stats_rate.py --trace-launches 5
  python scripts/read_stats_rate.py [--reads 2000000] --kernel-stats <dir>/.../run_kernel_stats.csv \\
      [--out profiles/read_stats_rate.txt]
"""
import argparse
import csv
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import fastkmer_amd as fk

K, M, B, READ_LEN, GENOME = 28, 10, 2048, 100, 100_000_000
LO, HI = 2, 0xFFFFFFFF  # the hit range of the report: solid = seen at least twice


def commit_hash() -> str:
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (not a git checkout)"


def kernel_resources() -> list[str]:
    path = os.path.join(os.path.dirname(fk.LIB_PATH), "kernel_resources.txt")
    if not os.path.exists(path):
        return ["kernel_resources.txt not found beside the library"]
    with open(path) as f:
        lines = f.read().splitlines()
    return [lines[0]] + [l for l in lines[1:] if "k_read_" in l]


def kernel_times(path: str) -> dict:
    """name -> (calls, total ns) of the traced run's k_query_seq and k_read_counts rows."""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for key in ("k_query_seq<1>", "k_read_counts<1>"):
                if key in r["Name"]:
                    out[key] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    return out


def host_stats(counts: np.ndarray, reads: np.ndarray) -> np.ndarray:
    """The caller's reduction: counts = fk_query_sequence over the reads joined by 'N' (101 positions a
    read), reads = the bases [n, 100].  Median by sort."""
    n, nw = len(reads), READ_LEN - K + 1
    c = np.concatenate([counts, np.zeros(READ_LEN + 1, dtype=np.uint32)])[:n * (READ_LEN + 1)]
    c = c.reshape(n, READ_LEN + 1)[:, :nw]
    bad = np.zeros((n, READ_LEN + 1), dtype=np.int16)
    np.cumsum(~np.isin(reads, np.frombuffer(b"ACGT", dtype=np.uint8)), axis=1, dtype=np.int16, out=bad[:, 1:])
    valid = bad[:, K:K + nw] == bad[:, :nw]
    out = np.zeros(n, dtype=fk.READ_STAT_DTYPE)
    w = valid.sum(axis=1)
    out["windows"] = w
    out["hits"] = (valid & (c >= LO) & (c <= HI)).sum(axis=1)
    out["sum"] = np.where(valid, c, 0).sum(axis=1, dtype=np.uint64)
    s = np.sort(np.where(valid, c, np.uint32(0xFFFFFFFF)), axis=1)
    rows, some = np.arange(n), w > 0
    out["min"] = np.where(some, s[:, 0], 0)
    out["median"] = np.where(some, s[rows, np.maximum(w - 1, 0) // 2], 0)
    out["max"] = np.where(some, s[rows, np.maximum(w - 1, 0)], 0)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-launches", type=int, default=0,
                    help="only run one fk_query_sequence and this many fk_read_counts_device launches (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="the kernel statistics CSV of a --trace-launches run")
    ap.add_argument("--commit", default=None, help="the commit hash to record (default: git rev-parse)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_stats_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("read_stats_rate.py measures on the GPU: none found")
    dev = torch.device("cuda")
    n = args.reads
    rec = READ_LEN + 14

    kc = fk.KmerCounter(K, M, 3, B)
    kc.synth_device(n, READ_LEN, GENOME, seed=0x5EED)
    kc.finish()
    st = kc.stats()

    # the job's reads as a CSR batch on the device, and joined by 'N' on the host
    text = torch.empty(n * rec, dtype=torch.uint8, device=dev)
    fk.synth_fasta_to_device(text.data_ptr(), n, READ_LEN, GENOME, seed=0x5EED)
    d_bases = text.view(n, rec)[:, 13:13 + READ_LEN].contiguous().view(-1)
    del text
    d_offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * READ_LEN
    nb = n * READ_LEN
    reads = d_bases.cpu().numpy().reshape(n, READ_LEN)
    joined = np.full((n, READ_LEN + 1), ord("N"), dtype=np.uint8)
    joined[:, :READ_LEN] = reads
    joined = joined.reshape(-1)[:-1].tobytes()

    d_counts = torch.empty(nb, dtype=torch.int32, device=dev)
    d_valid = torch.empty(nb, dtype=torch.uint8, device=dev)
    d_stats = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    scratch = torch.empty(fk.read_stats_scratch_bytes(nb), dtype=torch.uint8, device=dev)
    kc.set_stream(torch.cuda.current_stream().cuda_stream)

    def counts_launch():
        kc.read_counts_ptr(d_bases.data_ptr(), d_offsets.data_ptr(), n, d_counts.data_ptr(), d_valid.data_ptr())

    def stats_launch():
        kc.read_stats_ptr(d_bases.data_ptr(), d_offsets.data_ptr(), n, scratch.data_ptr(), scratch.numel(),
                          d_stats.data_ptr(), min_count=LO)

    if args.trace_launches:
        kc.query_sequence(joined)
        for _ in range(args.trace_launches):
            counts_launch()
        torch.cuda.synchronize()
        kc.close()
        return

    times = {}

    def measure(name, launch):
        for _ in range(args.warmup):
            launch()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.launches + 1)]
        evs[0].record()
        for i in range(args.launches):
            launch()
            evs[i + 1].record()
        torch.cuda.synchronize()
        times[name] = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.launches))

    measure("fk_read_counts_device", counts_launch)
    measure("fk_read_stats_device", stats_launch)
    dev_stats = d_stats.cpu().numpy().view(fk.READ_STAT_DTYPE)
    windows = int(dev_stats["windows"].sum())

    t0 = time.perf_counter()
    seq_counts = kc.query_sequence(joined)
    t_query = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = host_stats(seq_counts, reads)
    t_reduce = time.perf_counter() - t0
    same = bool(np.array_equal(ref, dev_stats))

    def line(name):
        t = times[name]
        med = t[len(t) // 2]
        return (f"{name}: median {med:.3f} ms per launch (min {t[0]:.3f}, max {t[-1]:.3f}, {args.launches} launches after "
                f"{args.warmup} warm-ups, device events) = {windows / med / 1e6:.2f} G windows/s, {n / med / 1e3:.1f} M reads/s")

    report = [
        "Per-read abundance profiles against the route through fk_query_sequence (scripts/read_stats_rate.py)",
        f"commit: {args.commit or commit_hash()}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"job: k={K} m={M} B={B}, {n} synthetic {READ_LEN} bp reads ({GENOME // 1_000_000} Mbp virtual genome): "
        f"{st['kmers']} k-mers, {st['distinct']} distinct",
        f"batch: the job's {n} reads, {nb} bases on the device, {windows} valid windows; hits = count >= {LO}",
        line("fk_read_counts_device"),
        line("fk_read_stats_device"),
        f"route without them: fk_query_sequence over the reads joined by 'N' ({len(joined)} bytes, one call) {t_query:.2f} s, "
        f"numpy reduction per read (median by sort) {t_reduce:.2f} s, together {t_query + t_reduce:.2f} s; one run, host clock",
        f"both routes give the same statistics: {same}",
    ]
    if args.kernel_stats:
        kt = kernel_times(args.kernel_stats)
        if len(kt) == 2:
            (qc, qt), (rc, rt) = kt["k_query_seq<1>"], kt["k_read_counts<1>"]
            report += [
                f"kernel time for those bases (rocprofv3 --kernel-trace --stats, a run of its own): k_query_seq<1> "
                f"{qt / 1e6:.3f} ms over {qc} launches of one fk_query_sequence call; k_read_counts<1> {rt / rc / 1e6:.3f} ms "
                f"per launch (mean of {rc}) = {qt / (rt / rc):.2f}x"]
        else:
            report += [f"kernel time: the statistics file holds {sorted(kt)} only"]
    else:
        report += ["kernel time against k_query_seq: not measured in this run (no --kernel-stats)"]
    report += ["profile kernels (kernel_resources.txt):", *["  " + l for l in kernel_resources()]]
    text = "\n".join(report) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    kc.close()
    if not same:
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
