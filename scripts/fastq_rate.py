"""FASTQ input against the FASTA headline: the normalise stage's device time and the FASTQ job's step time.

The reads of the configs[1] job (k=28 m=10 B=2048, ~1 GB of synthetic FASTA, 114 B a record) are
written as FASTQ (217 B a record: "@r%010d\\n", 100 bases, "+\\n", 100 qualities of Phred 2..40 at
offset 33, newlines) on the device and staged to pinned host memory, as bench.py stages its FASTA.

  * the normalise launches (fk_debug_fastq_ms: device events around each launch pair, summed over
    the job) for the whole input in one range (FASTKMER_INGEST_SEG above the input's size), summed
    over the streamed job (default segments), and for the out-of-place stage of fk_ingest_device;
    min_quality 0 and 20; in ms per GB of FASTQ and as a share of the 8 TB/s HBM roofline for the
    bytes the stage is meant to move: the range once, 4 B a line of index written and read, and the
    quality bytes again when masking (the out-of-place stage also writes the range once);
  * the FASTQ job's step time (fk_ingest from pinned memory + fk_finish, host clock around work that
    ends in a device synchronise): median of --steps after --warmup;
  * bench.py's headline on a checkout of the parent commit (--parent-tree, built) and on this tree,
    --bench-runs runs each, alternating, before this process opens the GPU;
  * the two conditions of the change: this tree's FASTA headline within the parent's own spread, and
    the FASTQ step at most 1.895 x the parent's FASTA step.

  python scripts/fastq_rate.py --parent-tree DIR [--out profiles/fastq_rate.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, M, B, READ_LEN, GENOME = 28, 10, 2048, 100, 100_000_000
FASTA_REC, FASTQ_REC = 114, 217
HBM_BYTES_PER_S = 8e12
BOUND = 1.895  # FASTQ step time over the parent's FASTA step time, as the change's issue sets it


def commit_hash() -> str:
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (not a git checkout)"


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def bench_ms(tree: str, steps: int, warmup: int) -> float:
    tree = os.path.abspath(tree)
    env = {k: v for k, v in os.environ.items() if k != "FASTKMER_LIB"}
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--no-cpu-baseline"], capture_output=True, text=True, env=env,
                       cwd=tree, timeout=600)
    if r.returncode != 0:
        sys.exit(f"bench.py in {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    ms = float(json.loads(line)["ms_per_step"])
    print(f"bench.py in {tree}: {ms:.3f} ms per step", file=sys.stderr, flush=True)
    return ms


def kernel_resources() -> list[str]:
    import fastkmer_amd as fk
    path = os.path.join(os.path.dirname(fk.LIB_PATH), "kernel_resources.txt")
    if not os.path.exists(path):
        return ["kernel_resources.txt not found beside the library"]
    with open(path) as f:
        lines = f.read().splitlines()
    return [lines[0]] + [l for l in lines[1:] if "k_fq_" in l]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000_000 // FASTA_REC)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit (its bench.py is run)")
    ap.add_argument("--parent-commit", default="", help="the parent's hash, for the report")
    ap.add_argument("--bench-runs", type=int, default=6)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_rate.txt"))
    args = ap.parse_args()

    # 1. the FASTA headline of both trees, alternating, before this process opens the GPU
    parent, tree = [], []
    for i in range(args.bench_runs if args.parent_tree else 0):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):  # parent first, then this tree first, ...
            (tree if which else parent).append(bench_ms(ROOT if which else args.parent_tree, args.bench_steps,
                                                        args.bench_warmup))

    import numpy as np  # noqa: F401
    import torch

    import fastkmer_amd as fk
    if not torch.cuda.is_available():
        sys.exit("fastq_rate.py measures on the GPU: none found")
    dev = torch.device("cuda")
    n = args.reads

    # 2. the job's reads as FASTQ, built on the device, staged to pinned memory
    fa = torch.empty(n * FASTA_REC, dtype=torch.uint8, device=dev)
    fk.synth_fasta_to_device(fa.data_ptr(), n, READ_LEN, GENOME, seed=0x5EED)
    fa = fa.view(n, FASTA_REC)
    fq = torch.empty((n, FASTQ_REC), dtype=torch.uint8, device=dev)
    fq[:, 0] = ord("@")
    fq[:, 1:114] = fa[:, 1:114]  # name, newline, bases, newline
    fq[:, 114] = ord("+")
    fq[:, 115] = ord("\n")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5EED)
    fq[:, 116:216] = torch.randint(2 + 33, 41 + 33, (n, READ_LEN), dtype=torch.uint8, device=dev, generator=gen)
    fq[:, 216] = ord("\n")
    low = int((fq[:, 116:216] < 20 + 33).sum().item())
    fq = fq.view(-1)
    nbytes = fq.numel()
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    host.copy_(fq)
    fa_host = torch.empty(n * FASTA_REC, dtype=torch.uint8, pin_memory=True)
    fa_host.copy_(fa.view(-1))
    del fa
    torch.cuda.synchronize()
    gb = nbytes / 1e9
    lines = 4 * n

    def stage_bytes(min_q, copy):
        return nbytes + 8 * lines + (READ_LEN * n if min_q else 0) + (nbytes if copy else 0)

    def job(kc, device_leg=False):
        t0 = time.perf_counter()
        if device_leg:
            kc.ingest_device(fq.data_ptr(), nbytes)
        else:
            kc.ingest_ptr(host.data_ptr(), nbytes)
        kc.finish()
        return (time.perf_counter() - t0) * 1e3

    # the FASTA job on this tree, through the same calls (its result is the FASTQ job's)
    with fk.KmerCounter(K, M, 3, B) as kc:
        kc.ingest_ptr(fa_host.data_ptr(), fa_host.numel())
        kc.finish()
        fa_st = kc.stats()
        fa_sizes = kc.bin_sizes()
    del fa_host

    rows, same = [], True
    step = {}
    for label, seg, device_leg in (("whole input in one range, in place", str(1 << 32), False),
                                   ("summed over the streamed job, in place", None, False),
                                   ("fk_ingest_device, out of place (one range)", None, True)):
        for min_q in (0, 20):
            if seg:
                os.environ["FASTKMER_INGEST_SEG"] = seg
            else:
                os.environ.pop("FASTKMER_INGEST_SEG", None)
            with fk.KmerCounter(K, M, 3, B, input_format="fastq", min_quality=min_q) as kc:
                for _ in range(args.warmup):
                    job(kc, device_leg)
                ts, ms = [], []
                for _ in range(args.steps):
                    ts.append(job(kc, device_leg))
                    ms.append(kc.fastq_stage_ms())
                info, st = kc.fastq_info(), kc.stats()
                if min_q == 0:
                    same = same and st["kmers"] == fa_st["kmers"] and st["distinct"] == fa_st["distinct"] and \
                        bool((kc.bin_sizes() == fa_sizes).all())
                same = same and info["records"] == n and info["first_malformed"] is None and \
                    info["masked_bases"] == (low if min_q else 0)
            med, lo, hi = stats([m[0] for m in ms])
            nb = stage_bytes(min_q, device_leg)
            rows.append(f"normalise, {label}, min_quality {min_q}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}; "
                        f"{ms[-1][1]} launches a job, {args.steps} jobs after {args.warmup} warm-ups, device events) = "
                        f"{med / gb:.3f} ms per GB of FASTQ; {nb} bytes to move = {nb / (med * 1e-3) / 1e12:.2f} TB/s = "
                        f"{100 * nb / (med * 1e-3) / HBM_BYTES_PER_S:.1f} % of the 8 TB/s HBM roofline")
            step[(label, min_q)] = stats(ts)
            print(rows[-1], file=sys.stderr, flush=True)
    os.environ.pop("FASTKMER_INGEST_SEG", None)

    def step_line(name, key):
        med, lo, hi = step[key]
        return (f"{name}: median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}, {args.steps} steps after {args.warmup} "
                f"warm-ups, host clock around fk_ingest + fk_finish)")

    fq_step = step[("summed over the streamed job, in place", 0)][0]
    report = [
        "FASTQ input: the normalise stage and the FASTQ job against the FASTA headline (scripts/fastq_rate.py)",
        f"commit: {args.commit or commit_hash()}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"job: k={K} m={M} B={B}, {n} synthetic {READ_LEN} bp reads: {n * FASTA_REC} bytes of FASTA, {nbytes} bytes of "
        f"FASTQ ({FASTQ_REC} B a record, {nbytes / (n * FASTA_REC):.3f}x the FASTA), {low} bases below Phred 20; "
        f"{fa_st['kmers']} k-mers, {fa_st['distinct']} distinct",
        f"the FASTQ jobs give the FASTA job's k-mers, distinct count and bin sizes, {n} records, no malformed record, "
        f"and the expected masked bases: {same}",
        *rows,
        step_line("FASTQ job step, pinned source, streamed (the bench's path), min_quality 0",
                  ("summed over the streamed job, in place", 0)),
        step_line("FASTQ job step, pinned source, streamed, min_quality 20", ("summed over the streamed job, in place", 20)),
        step_line("FASTQ job step, fk_ingest_device, min_quality 0", ("fk_ingest_device, out of place (one range)", 0)),
    ]
    if parent:
        p_med, p_lo, p_hi = stats(parent)
        t_med, t_lo, t_hi = stats(tree)
        within = p_lo <= t_med <= p_hi
        report += [
            f"bench.py headline (--gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}), parent "
            f"{args.parent_commit or 'commit'}: ms_per_step " + ", ".join(f"{x:.3f}" for x in parent) +
            f" (median {p_med:.3f}, spread {p_lo:.3f} .. {p_hi:.3f})",
            "bench.py headline, this tree (runs alternating with the parent's, either one first in turn): ms_per_step " +
            ", ".join(f"{x:.3f}" for x in tree) + f" (median {t_med:.3f}, spread {t_lo:.3f} .. {t_hi:.3f})",
            f"condition 1, the FASTA headline of this tree lies within the parent's own spread: "
            f"{'holds' if within else 'FAILS'} ({t_med:.3f} against {p_lo:.3f} .. {p_hi:.3f})",
            f"condition 2, the FASTQ step is at most {BOUND} x the parent's FASTA step: "
            f"{'holds' if fq_step <= BOUND * p_med else 'FAILS'} ({fq_step:.2f} ms against {BOUND} x {p_med:.3f} = "
            f"{BOUND * p_med:.2f} ms; ratio {fq_step / p_med:.3f})",
        ]
    else:
        report.append("bench.py headline of the parent commit: not measured (no --parent-tree)")
    report += ["stage kernels (kernel_resources.txt):", *["  " + l for l in kernel_resources()]]
    text = "\n".join(report) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    if not same:
        sys.exit("a FASTQ job disagrees with the FASTA job")


if __name__ == "__main__":
    main()
