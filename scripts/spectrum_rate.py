"""The abundance spectrum on the device (fk_spectrum_device, fk_spectrum) against the only route without
it -- every bin copied to the host (fk_get_bin) and np.bincount there -- and fk_write_bins_range(2, max)
against fk_write_bins.

A configs[1]-parameter job (k=28 m=10 B=2048) of --reads synthetic reads is counted on the device.
fk_spectrum_device is timed with device events on the context's stream over --launches launches after
--warmup warm-ups, for n = 256 and n = 65536; fk_spectrum (host arrays filled) and the host route
with the host clock, --repeats runs each after one warm-up; medians are reported with min and max.
Both routes must give the same spectrum.  The kernel's bytes are the counts (4 per distinct k-mer) and
the bucket metadata it walks (8 bytes of Bucket.begin and the dense_off pair per bucket); the roofline
fraction is those bytes over the median time against 8 TB/s.  The two writers go to a directory in
memory (--tmp, default /dev/shm), --repeats runs each, with the k-mers (lines) and bytes they wrote.
Writes a small report (--out).

  python scripts/spectrum_rate.py [--reads 2000000] [--out profiles/spectrum_rate.txt]
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

import numpy as np
import torch

import fastkmer_amd as fk

K, M, B, READ_LEN, GENOME = 28, 10, 2048, 100, 100_000_000
HBM_BYTES_PER_S = 8e12


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
    return [lines[0]] + [l for l in lines[1:] if "k_spectrum" in l or "k_range" in l]


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def dir_bytes(d):
    names = os.listdir(d)
    return len(names), sum(os.path.getsize(os.path.join(d, f)) for f in names)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--commit", default=None, help="the commit hash to record (default: git rev-parse)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spectrum_rate.py measures on the GPU: none found")
    dev = torch.device("cuda")

    kc = fk.KmerCounter(K, M, 3, B)
    kc.synth_device(args.reads, READ_LEN, GENOME, seed=0x5EED)
    kc.finish()
    st = kc.stats()
    sizes = kc.bin_sizes()
    distinct, nbuckets = int(st["distinct"]), int(st["buckets"])
    kc.set_stream(torch.cuda.current_stream().cuda_stream)

    # 1. the device form, device events around every launch
    dev_ms, dev_hist = {}, {}
    d_tail = torch.zeros(1, dtype=torch.int64, device=dev)
    for n in (256, 65536):
        d_hist = torch.zeros(n, dtype=torch.int64, device=dev)
        for _ in range(args.warmup):
            kc.spectrum_ptr(d_hist.data_ptr(), n, d_tail.data_ptr())
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.launches + 1)]
        evs[0].record()
        for i in range(args.launches):
            kc.spectrum_ptr(d_hist.data_ptr(), n, d_tail.data_ptr())
            evs[i + 1].record()
        torch.cuda.synchronize()
        dev_ms[n] = stats([evs[i].elapsed_time(evs[i + 1]) for i in range(args.launches)])
        dev_hist[n] = d_hist.cpu().numpy().view(np.uint64)

    # 2. the host form
    kc.spectrum(256)
    host_form = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        hist = kc.spectrum(256)
        host_form.append((time.perf_counter() - t0) * 1e3)
    host_form = stats(host_form)

    # 3. the route of the parent commit: every bin through fk_get_bin, np.bincount on the host
    def host_route(n):
        t0 = time.perf_counter()
        acc = np.zeros(n, dtype=np.int64)
        for b in range(B):
            if sizes[b]:
                acc += np.bincount(np.minimum(kc.get_bin(b)[1], n - 1), minlength=n)
        return acc.astype(np.uint64), (time.perf_counter() - t0) * 1e3

    host_route(256)
    route = []
    for _ in range(args.repeats):
        ref_hist, ms = host_route(256)
        route.append(ms)
    route = stats(route)
    same = bool(np.array_equal(ref_hist, hist) and np.array_equal(ref_hist, dev_hist[256]) and
                np.array_equal(host_route(65536)[0], dev_hist[65536]))

    # 4. the writers, into memory
    tmp = tempfile.mkdtemp(prefix="fk_spectrum_rate_", dir=args.tmp)
    written = {}
    try:
        for name, kw in (("fk_write_bins", {}), ("fk_write_bins_range(2, max)", {"min_count": 2})):
            ts = []
            for i in range(args.repeats + 1):
                d = os.path.join(tmp, "out")
                t0 = time.perf_counter()
                kc.write_bins(d, **kw)
                if i:  # the first run warms up
                    ts.append((time.perf_counter() - t0) * 1e3)
                files, nbytes = dir_bytes(d)
                shutil.rmtree(d)
            kmers = int(kc.bin_sizes(**kw).sum())
            written[name] = (stats(ts), files, nbytes, kmers)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    bytes_read = 4 * distinct + 24 * nbuckets
    med256, med64k = dev_ms[256][0], dev_ms[65536][0]
    w_all, w_rng = written["fk_write_bins"], written["fk_write_bins_range(2, max)"]

    def dev_line(n):
        med, lo, hi = dev_ms[n]
        return (f"fk_spectrum_device (n = {n}): median {med:.3f} ms per launch (min {lo:.3f}, max {hi:.3f}, "
                f"{args.launches} launches after {args.warmup} warm-ups, device events) = {distinct / med / 1e6:.1f} G k-mers/s, "
                f"{bytes_read / (med * 1e-3) / 1e12:.2f} TB/s = {100 * bytes_read / (med * 1e-3) / HBM_BYTES_PER_S:.0f} % "
                f"of the 8 TB/s HBM roofline")

    def write_line(name):
        (med, lo, hi), files, nbytes, kmers = written[name]
        return (f"{name}: median {med:.0f} ms (min {lo:.0f}, max {hi:.0f}, {args.repeats} runs after 1 warm-up, host clock), "
                f"{kmers} k-mers in {files} files, {nbytes} bytes")

    report = [
        "Abundance spectrum on the device against the host route; bin files with a count range (scripts/spectrum_rate.py)",
        f"commit: {args.commit or commit_hash()}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"job: k={K} m={M} B={B}, {args.reads} synthetic {READ_LEN} bp reads ({GENOME // 1_000_000} Mbp virtual genome): "
        f"{st['kmers']} k-mers, {distinct} distinct, {nbuckets} buckets, F = {st['fine_bits']}",
        f"spectrum (c: distinct k-mers): " + ", ".join(f"{c}: {int(hist[c])}" for c in range(1, 9)) +
        f"; {100 * int(hist[1]) / max(distinct, 1):.1f} % singletons",
        f"bytes the spectrum kernel reads: 4 per distinct k-mer + 24 per bucket (Bucket.begin, dense_off pair) = {bytes_read}",
        dev_line(256),
        dev_line(65536),
        f"fk_spectrum (n = 256, host arrays filled): median {host_form[0]:.3f} ms (min {host_form[1]:.3f}, max {host_form[2]:.3f}, "
        f"{args.repeats} runs after 1 warm-up, host clock)",
        f"host route (fk_get_bin of every bin + np.bincount, n = 256): median {route[0]:.0f} ms (min {route[1]:.0f}, "
        f"max {route[2]:.0f}, {args.repeats} runs after 1 warm-up, host clock)",
        f"host route / fk_spectrum_device (n = 256): {route[0] / med256:.0f}x; host route / fk_spectrum: {route[0] / host_form[0]:.0f}x; "
        f"n = 65536 / n = 256 on the device: {med64k / med256:.2f}x",
        f"host route, fk_spectrum and fk_spectrum_device give the same spectrum (n = 256 and n = 65536): {same}",
        "writers into memory (fk_write_bins keeps its dense copy of the result from the warm-up run; the range form "
        "filters and compacts in every run):",
        write_line("fk_write_bins"),
        write_line("fk_write_bins_range(2, max)"),
        f"fk_write_bins_range(2, max) / fk_write_bins: {w_rng[0][0] / w_all[0][0]:.2f}x the time for "
        f"{w_rng[3] / max(w_all[3], 1):.2f}x the k-mers and {w_rng[2] / max(w_all[2], 1):.2f}x the bytes",
        "spectrum and range kernels (kernel_resources.txt):",
        *["  " + l for l in kernel_resources()],
    ]
    text = "\n".join(report) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    kc.close()
    if not same:
        sys.exit("the host route and the device spectrum disagree")


if __name__ == "__main__":
    main()
