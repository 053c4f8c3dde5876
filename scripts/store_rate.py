"""fk_save / fk_load of a counted result against what there was before them: fk_write_bins (the only
persistence) and a recount of the sample's FASTA from pinned memory (the only way to get a result back).

A configs[1]-parameter job (k=28 m=10 B=2048) of --reads synthetic reads is counted on the device and
saved to --tmp (default /dev/shm: the file stays in memory, so the load reads the page cache), --repeats
runs of each call after one warm-up, medians with min and max.  The splits are the library's own
(fk_debug_store_ms): device events around the export and checksum, the H2D of the sections and the
import's three steps; the host clock around the waits for the copy windows, the file reads and the writes.
The one comparison the import has to stand: its device time (verify + cell offsets + bucket tables)
against fk_query_device over the same keys in the same run (--launches launches, device events) -- both
scan every key's m-mers, the import without the lookups' dependent loads.  The loaded context must hold
the saved result (export arrays equal).  Writes a small report (--out).

  python scripts/store_rate.py [--reads 2000000] [--out profiles/store_rate.txt]
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

import fastkmer_amd as fk

K, M, B, READ_LEN, GENOME = 28, 10, 2048, 100, 100_000_000


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
    return [lines[0]] + [l for l in lines[1:] if "k_store" in l or "k_queryILi1" in l]


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(name, ts, unit="ms"):
    m, lo, hi = med(ts)
    return f"{name}: median {m:.1f} {unit} (min {lo:.1f}, max {hi:.1f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--commit", default=None, help="the commit hash to record (default: git rev-parse)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("store_rate.py measures on the GPU: none found")
    dev = torch.device("cuda")

    kc = fk.KmerCounter(K, M, 3, B)
    nbytes = kc.synth_device(args.reads, READ_LEN, GENOME, seed=0x5EED)
    kc.finish()
    st = kc.stats()
    distinct = int(st["distinct"])
    tmp = tempfile.mkdtemp(prefix="fk_store_rate_", dir=args.tmp)
    path = os.path.join(tmp, "sample.fkdb")
    try:
        # 1. fk_save
        save = {n: [] for n in ("wall", "device_copy", "host_copy_or_read", "write")}
        for i in range(args.repeats + 1):
            kc.save(path)
            if i:
                for n, v in kc.store_ms().items():
                    if n in save:
                        save[n].append(v)
        file_bytes = os.path.getsize(path)
        # 2. fk_load of the file in the page cache, into a context of its own
        ld = fk.KmerCounter(K, M, 3, B)
        load = {n: [] for n in ("wall", "device_copy", "host_copy_or_read", "verify", "cells", "buckets")}
        for i in range(args.repeats + 1):
            ld.load_into(path)
            if i:
                for n, v in ld.store_ms().items():
                    if n in load:
                        load[n].append(v)
        lst = ld.stats()
        # 3. the loaded context holds the saved result; fk_query_device over the same keys in the same run
        d_keys = torch.zeros(distinct, dtype=torch.int64, device=dev)
        d_counts = torch.zeros(distinct, dtype=torch.int32, device=dev)
        d_got = torch.zeros(distinct, dtype=torch.int32, device=dev)
        l_keys = torch.zeros(distinct, dtype=torch.int64, device=dev)
        l_counts = torch.zeros(distinct, dtype=torch.int32, device=dev)
        assert kc.export_ptr(d_keys.data_ptr(), d_counts.data_ptr(), distinct) == distinct
        assert ld.export_ptr(l_keys.data_ptr(), l_counts.data_ptr(), distinct) == distinct
        torch.cuda.synchronize()
        same = bool(torch.equal(d_keys, l_keys) and torch.equal(d_counts, l_counts))
        del l_keys, l_counts
        ld.set_stream(torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            ld.query_ptr(d_keys.data_ptr(), distinct, d_got.data_ptr())
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.launches + 1)]
        evs[0].record()
        for i in range(args.launches):
            ld.query_ptr(d_keys.data_ptr(), distinct, d_got.data_ptr())
            evs[i + 1].record()
        torch.cuda.synchronize()
        query = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.launches)]
        same = same and bool(torch.equal(d_got, d_counts))
        ld.close()
        del d_keys, d_counts, d_got
        # 4. what there was before: the text bin files, and a recount of the FASTA from pinned memory
        bins_ms, bins_bytes = [], 0
        for i in range(args.repeats + 1):
            d = os.path.join(tmp, "bins")
            t0 = time.perf_counter()
            kc.write_bins(d)
            if i:
                bins_ms.append((time.perf_counter() - t0) * 1e3)
            bins_bytes = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
            shutil.rmtree(d)
        fasta = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        fk.synth_fasta_to_device(fasta.data_ptr(), args.reads, READ_LEN, GENOME, seed=0x5EED)
        pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        pinned.copy_(fasta)
        torch.cuda.synchronize()
        del fasta
        rc = fk.KmerCounter(K, M, 3, B)
        recount = []
        for i in range(args.repeats + 1):
            t0 = time.perf_counter()
            rc.ingest_ptr(pinned.data_ptr(), nbytes)
            rc.finish()
            if i:
                recount.append((time.perf_counter() - t0) * 1e3)
        same = same and rc.stats()["distinct"] == distinct
        rc.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    imp = [a + b + c for a, b, c in zip(load["verify"], load["cells"], load["buckets"])]
    report = [
        "fk_save / fk_load of a counted result; fk_write_bins and a recount for comparison (scripts/store_rate.py)",
        f"commit: {args.commit or commit_hash()}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"job: k={K} m={M} B={B}, {args.reads} synthetic {READ_LEN} bp reads ({GENOME // 1_000_000} Mbp virtual genome, "
        f"{nbytes} FASTA bytes): {st['kmers']} k-mers, {distinct} distinct, {st['buckets']} buckets, F = {st['fine_bits']}",
        f"database file: {file_bytes} bytes in {args.tmp or 'the default temporary directory'} (12 bytes per distinct k-mer and the "
        f"header); the imported result: {lst['buckets']} buckets, F = {lst['fine_bits']}",
        f"every figure: {args.repeats} runs after 1 warm-up",
        fmt("fk_save, wall (host clock)", save["wall"]),
        fmt("  export + checksum (device events)", save["device_copy"]),
        fmt("  waits for the D2H windows (host clock; the copies overlap the writes)", save["host_copy_or_read"]),
        fmt("  file writes (host clock)", save["write"]),
        f"  = {file_bytes / med(save['wall'])[0] / 1e6:.2f} GB/s of file",
        fmt("fk_load from the page cache, wall (host clock)", load["wall"]),
        fmt("  file reads (host clock)", load["host_copy_or_read"]),
        fmt("  H2D of the sections, first copy queued to last landed (device events; spans the reads)", load["device_copy"]),
        fmt("  import: verify (device events)", load["verify"]),
        fmt("  import: cell offsets (device events)", load["cells"]),
        fmt("  import: bucket tables (device events)", load["buckets"]),
        f"  = {file_bytes / med(load['wall'])[0] / 1e6:.2f} GB/s of file",
        fmt("the import's device time (verify + cell offsets + bucket tables)", imp),
        fmt(f"fk_query_device over the same {distinct} keys in the same run ({args.launches} launches, device events)", query),
        f"import device time / fk_query_device: {med(imp)[0] / med(query)[0]:.2f}x",
        fmt(f"fk_write_bins of the same result ({bins_bytes} bytes of text), host clock", bins_ms),
        fmt("recount of the sample's FASTA from pinned memory (fk_ingest + fk_finish, the count's code is the parent "
            "commit's), host clock", recount),
        f"fk_load / recount: {med(load['wall'])[0] / med(recount)[0]:.1f}x the time",
        f"the loaded context exports the saved arrays, fk_query_device finds every key with its count, the recount has "
        f"as many distinct k-mers: {same}",
        "kernels (kernel_resources.txt):",
        *["  " + l for l in kernel_resources()],
    ]
    text = "\n".join(report) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    kc.close()
    if not same:
        sys.exit("the loaded result differs from the saved one")


if __name__ == "__main__":
    main()
