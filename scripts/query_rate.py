"""The rate of device lookups (fk_query_device) against the only route without them: every bin copied
to the host (fk_get_bin) and searched there.

A configs[1]-parameter job (k=28 m=10 B=2048) of --reads synthetic reads is counted on the device;
--queries keys are made on the device, half drawn from sampled bins of the result (hits, half of them
turned to the other strand), half uniform random (misses).  The device path is timed with device
events over --launches launches after --warmup warm-ups, and once more with the hits drawn from
every bin (the sampled bins' keys fit the caches, the whole result does not).  The host route is
timed once: fk_get_bin of every bin, then canonical keys grouped by bin and one np.searchsorted per
bin; it takes the queries' bins from the device answer, so the bin computation a real caller of that
route would also need is not in its time.  Both routes must give the same counts.  Writes a small
report (--out).

  python scripts/query_rate.py [--reads 2000000] [--queries 33554432] [--out profiles/query_rate.txt]
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
U64 = np.uint64


def revcomp64(x: np.ndarray, k: int) -> np.ndarray:
    x = ~x
    x = ((x >> U64(2)) & U64(0x3333333333333333)) | ((x & U64(0x3333333333333333)) << U64(2))
    x = ((x >> U64(4)) & U64(0x0F0F0F0F0F0F0F0F)) | ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4))
    return x.byteswap() >> U64(64 - 2 * k)


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
    return [lines[0]] + [l for l in lines[1:] if "k_query" in l]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--queries", type=int, default=32 << 20)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample-bins", type=int, default=64)
    ap.add_argument("--commit", default=None, help="the commit hash to record (default: git rev-parse)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("query_rate.py measures on the GPU: none found")
    dev = torch.device("cuda")
    n = args.queries

    kc = fk.KmerCounter(K, M, 3, B)
    kc.synth_device(args.reads, READ_LEN, GENOME, seed=0x5EED)
    kc.finish()
    st = kc.stats()
    sizes = kc.bin_sizes()

    # the route without lookups starts with every bin on the host
    t0 = time.perf_counter()
    table = [kc.get_bin(b) if sizes[b] else None for b in range(B)]
    t_copy = time.perf_counter() - t0

    # queries: hits from a pool of stored keys (every other one on the other strand), uniform random misses
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED)

    def make_queries(pool_bins):
        pool = np.concatenate([table[b][0] for b in pool_bins if table[b] is not None])
        pool[1::2] = revcomp64(pool[1::2], K)
        d_pool = torch.from_numpy(pool.view(np.int64)).to(dev)
        hits = d_pool[torch.randint(0, len(pool), (n // 2,), device=dev, generator=g)]
        misses = torch.randint(0, 1 << (2 * K), (n - n // 2,), dtype=torch.int64, device=dev, generator=g)
        return torch.cat([hits, misses])[torch.randperm(n, device=dev, generator=g)].contiguous()

    d_counts = torch.empty(n, dtype=torch.int32, device=dev)
    d_bins = torch.empty(n, dtype=torch.int32, device=dev)
    kc.set_stream(torch.cuda.current_stream().cuda_stream)
    times = {}

    def measure(name, d_keys, bins_ptr):
        for _ in range(args.warmup):
            kc.query_ptr(d_keys.data_ptr(), n, d_counts.data_ptr(), bins_ptr)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.launches + 1)]
        evs[0].record()
        for i in range(args.launches):
            kc.query_ptr(d_keys.data_ptr(), n, d_counts.data_ptr(), bins_ptr)
            evs[i + 1].record()
        torch.cuda.synchronize()
        times[name] = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.launches))

    d_spread = make_queries(range(B))
    measure("hits from every bin, counts + bins", d_spread, d_bins.data_ptr())
    found_spread = int(torch.count_nonzero(d_counts))
    del d_spread
    d_keys = make_queries(np.linspace(0, B - 1, args.sample_bins).astype(np.int64).tolist())
    measure("counts only", d_keys, 0)
    measure("counts + bins", d_keys, d_bins.data_ptr())
    counts = d_counts.cpu().numpy().view(np.uint32)
    bins = d_bins.cpu().numpy()
    keys = d_keys.cpu().numpy().view(U64)

    # ... then the queries' canonical keys grouped by bin and searched in the bin's sorted keys
    t0 = time.perf_counter()
    canon = np.minimum(keys, revcomp64(keys, K))
    order = np.argsort(bins, kind="stable")
    cuts = np.searchsorted(bins[order], np.arange(B + 1))
    host = np.zeros(n, dtype=np.uint32)
    for b in range(B):
        idx = order[cuts[b]:cuts[b + 1]]
        if table[b] is None or len(idx) == 0:
            continue
        bk, bc = table[b]
        q = canon[idx]
        pos = np.minimum(np.searchsorted(bk, q), len(bk) - 1)
        host[idx] = np.where(bk[pos] == q, bc[pos], 0)
    t_host = t_copy + time.perf_counter() - t0
    same = bool(np.array_equal(host, counts))

    def line(name):
        t = times[name]
        med = t[len(t) // 2]
        return (f"fk_query_device ({name}): median {med:.3f} ms per launch of {n} keys (min {t[0]:.3f}, max {t[-1]:.3f}, "
                f"{args.launches} launches after {args.warmup} warm-ups, device events) = {n / med / 1e6:.2f} G queries/s")

    report = [
        "Device lookups against the host route (scripts/query_rate.py)",
        f"commit: {args.commit or commit_hash()}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"job: k={K} m={M} B={B}, {args.reads} synthetic {READ_LEN} bp reads ({GENOME // 1_000_000} Mbp virtual genome): "
        f"{st['kmers']} k-mers, {st['distinct']} distinct, {st['buckets']} buckets, F = {st['fine_bits']}",
        f"queries: {n} keys on the device, half from {args.sample_bins} sampled bins (every other one reverse-"
        f"complemented), half uniform random; {int(np.count_nonzero(counts))} found",
        line("counts + bins"),
        line("counts only"),
        f"the same with the hits drawn from every bin ({found_spread} found):",
        line("hits from every bin, counts + bins"),
        f"host route (every bin through fk_get_bin, then np.searchsorted per bin; bins taken from the device answer): "
        f"{t_host:.2f} s, of it {t_copy:.2f} s copying {int(sizes.sum())} keys and counts out; one run, host clock",
        f"host route and device path give the same counts: {same}",
        "lookup kernels (kernel_resources.txt):",
        *["  " + l for l in kernel_resources()],
    ]
    text = "\n".join(report) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    kc.close()
    if not same:
        sys.exit("the host route and the device path disagree")


if __name__ == "__main__":
    main()
