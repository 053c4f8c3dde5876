"""The joint count matrix of two counted samples on the device (fk_compare_device, fk_compare) against
the only route without it -- every bin of each context copied to the host (fk_get_bin), its keys looked
up in the other context (fk_query) and np.add.at there -- and against fk_query_device over the same keys,
the yardstick of the kernel: the comparison does the same lookups, with sorted instead of arbitrary
keys, plus a count read and a histogram update.

Two configs[1]-parameter jobs (k=28 m=10 B=2048) of --reads synthetic reads each are counted on the
device: the same seed and genome, the second sample's reads starting half a sample later, so half of
the reads are shared.  (a) fk_compare_device is timed with device events on the context's stream over
--launches launches after --warmup warm-ups (both walks together); (b) fk_compare (host matrix filled)
and (c) the host route with the host clock, --repeats runs each after one warm-up; (d) fk_query_device
of A's dense keys in B plus B's dense keys in A, device events, the two launches of a round summed.
Medians are reported with min and max.  All routes must give the same matrix.  Writes a small report
(--out).

  python scripts/compare_rate.py [--reads 2000000] [--out profiles/compare_rate.txt]
"""
import argparse
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
N = 256  # rows = cols of the matrix


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
    return [lines[0]] + [l for l in lines[1:] if "k_compare" in l or "k_join" in l or "k_query" in l]


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(s, unit="ms", digits=3):
    return f"median {s[0]:.{digits}f} {unit} (min {s[1]:.{digits}f}, max {s[2]:.{digits}f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit hash to record (default: git rev-parse)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("compare_rate.py measures on the GPU: none found")
    dev = torch.device("cuda")

    ka, kb = fk.KmerCounter(K, M, 3, B), fk.KmerCounter(K, M, 3, B)
    ka.synth_device(args.reads, READ_LEN, GENOME, seed=0x5EED)
    ka.finish()
    kb.synth_device(args.reads, READ_LEN, GENOME, seed=0x5EED, first_read=args.reads // 2)
    kb.finish()
    sa, sb = ka.stats(), kb.stats()
    stream = torch.cuda.current_stream().cuda_stream
    ka.set_stream(stream)
    kb.set_stream(stream)

    def timed(launch):
        for _ in range(args.warmup):
            launch()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.launches + 1)]
        evs[0].record()
        for i in range(args.launches):
            launch()
            evs[i + 1].record()
        torch.cuda.synchronize()
        return stats([evs[i].elapsed_time(evs[i + 1]) for i in range(args.launches)])

    # (a) the device form, both walks between two events
    d_mat = torch.zeros(N * N, dtype=torch.int64, device=dev)
    dev_ms = timed(lambda: ka.compare_ptr(kb, d_mat.data_ptr(), N, N))
    dev_mat = d_mat.cpu().numpy().view(np.uint64).reshape(N, N)
    d_big = torch.zeros(4096 * 4096, dtype=torch.int64, device=dev)
    big_ms = timed(lambda: ka.compare_ptr(kb, d_big.data_ptr(), 4096, 4096))
    self_ms = timed(lambda: ka.compare_ptr(ka, d_mat.data_ptr(), N, N))

    # (b) the host form
    ka.compare(kb, N, N)
    host_form = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        mat = ka.compare(kb, N, N)
        host_form.append((time.perf_counter() - t0) * 1e3)
    host_form = stats(host_form)

    # (c) the route of the parent commit: every bin of each context through fk_get_bin, its keys through
    # the other's fk_query, np.add.at on the host; the k-mers found by the second pass were counted by the first
    dense = [None, None]

    def host_route():
        t0 = time.perf_counter()
        acc = np.zeros((N, N), dtype=np.uint64)
        for side, (x, y) in enumerate(((ka, kb), (kb, ka))):
            sizes = x.bin_sizes()
            keys, counts = [], []
            for b in range(B):
                if sizes[b]:
                    kk, cc = x.get_bin(b)
                    keys.append(kk), counts.append(cc)
            keys, counts = np.concatenate(keys), np.concatenate(counts)
            other = y.query(keys)
            dense[side] = keys
            if side == 0:
                np.add.at(acc, (np.minimum(counts, N - 1), np.minimum(other, N - 1)), 1)
            else:
                absent = other == 0
                np.add.at(acc, (np.zeros(int(absent.sum()), dtype=np.int64), np.minimum(counts[absent], N - 1)), 1)
        return acc, (time.perf_counter() - t0) * 1e3

    host_route()
    route = []
    for _ in range(args.repeats):
        ref_mat, ms = host_route()
        route.append(ms)
    route = stats(route)
    same = bool(np.array_equal(ref_mat, mat) and np.array_equal(ref_mat, dev_mat))

    # (d) the yardstick: fk_query_device over the same two sets of dense keys, on the device already
    d_keys = [torch.from_numpy(k.view(np.int64)).to(dev) for k in dense]
    d_counts = [torch.zeros(len(k), dtype=torch.int32, device=dev) for k in dense]

    def query_both():
        ka.query_ptr(d_keys[1].data_ptr(), len(dense[1]), d_counts[1].data_ptr())
        kb.query_ptr(d_keys[0].data_ptr(), len(dense[0]), d_counts[0].data_ptr())

    query_ms = timed(query_both)
    found = int((d_counts[0] != 0).sum())
    same_lookups = bool(found == int(dev_mat[1:, 1:].sum()) == int((d_counts[1] != 0).sum()))

    ratio = dev_ms[0] / query_ms[0]
    n_keys = len(dense[0]) + len(dense[1])
    report = [
        "Joint count matrix of two samples on the device against the host route and against the lookups alone "
        "(scripts/compare_rate.py)",
        f"commit: {args.commit or commit_hash()}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"jobs: k={K} m={M} B={B}, two samples of {args.reads} synthetic {READ_LEN} bp reads of one {GENOME // 1_000_000} Mbp "
        f"virtual genome, the second starting at read {args.reads // 2} (half of the reads shared)",
        f"sample A: {sa['kmers']} k-mers, {sa['distinct']} distinct, {sa['buckets']} buckets, F = {sa['fine_bits']}; "
        f"sample B: {sb['kmers']} k-mers, {sb['distinct']} distinct, {sb['buckets']} buckets, F = {sb['fine_bits']}",
        f"matrix ({N} x {N}): {int(mat[1:, 1:].sum())} k-mers in both, {int(mat[1:, 0].sum())} only in A, "
        f"{int(mat[0, 1:].sum())} only in B; M[1][0] = {int(mat[1, 0])}, M[0][1] = {int(mat[0, 1])}, M[1][1] = {int(mat[1, 1])}, "
        f"M[2][2] = {int(mat[2, 2])}",
        f"(a) fk_compare_device ({N} x {N}, both walks, {n_keys} lookups): {fmt(dev_ms)} per call, {args.launches} calls after "
        f"{args.warmup} warm-ups, device events = {n_keys / dev_ms[0] / 1e6:.2f} G lookups/s",
        f"    fk_compare_device (4096 x 4096, the 128 MB matrix cleared in every call): {fmt(big_ms)}",
        f"    fk_compare_device (A against itself, one walk, {N} x {N}): {fmt(self_ms)}",
        f"(b) fk_compare ({N} x {N}, host matrix filled): {fmt(host_form)}, {args.repeats} runs after 1 warm-up, host clock",
        f"(c) host route (fk_get_bin of every bin of both contexts + fk_query in the other + np.add.at): "
        f"{fmt(route, digits=0)}, {args.repeats} runs after 1 warm-up, host clock",
        f"(d) fk_query_device of A's {len(dense[0])} dense keys in B plus B's {len(dense[1])} in A (two launches): "
        f"{fmt(query_ms)} per pair, {args.launches} pairs after {args.warmup} warm-ups, device events = "
        f"{n_keys / query_ms[0] / 1e6:.2f} G lookups/s",
        f"(c) / (a): {route[0] / dev_ms[0]:.0f}x; (c) / (b): {route[0] / host_form[0]:.0f}x; (a) / (d): {ratio:.2f}x "
        f"(expected: at most 1.10x)" + ("" if ratio <= 1.10 else " -- SLOWER than the yardstick allows"),
        f"host route, fk_compare and fk_compare_device give the same matrix: {same}; the lookups of (d) find the "
        f"k-mers the matrix holds off row 0 and column 0: {same_lookups}",
        "comparison and lookup kernels (kernel_resources.txt):",
        *["  " + l for l in kernel_resources()],
    ]
    text = "\n".join(report) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    ka.close()
    kb.close()
    if not (same and same_lookups):
        sys.exit("the routes disagree")


if __name__ == "__main__":
    main()
