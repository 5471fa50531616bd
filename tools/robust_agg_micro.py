"""Micro-benchmark of the robust-aggregation kernels against the torch
composition they replace, on the GPU.

  rank_mean_rows(rows, lo, hi)   vs  stack + sort(0) + slice-mean
  pairwise_sqdist_rows(rows)     vs  stack + cdist(x, x)**2 (fp32)

Sizes: n = 11,173,962 (the flagship ResNet-18 flat vector) and n = 1M, with
K in {4, 8, 16, 32, 64}. Each repetition is bracketed by device events and runs
the op often enough to last about 20 ms; the two sides alternate within a
repetition. Reported: median ms per call, min..max over the repetitions
(the spread), achieved GB/s of the K*n*4 bytes the problem needs, and the
ratio torch/ours.

    python tools/robust_agg_micro.py [--reps 7] [--misaligned] [--out table.md]
"""
from __future__ import annotations

import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from fl4health_amd.ops import functional as F  # noqa: E402

SIZES = (11_173_962, 1_000_000)
KS = (4, 8, 16, 32, 64)
TARGET_MS = 20.0
PEAK_COPY_TBS = 6.29  # measured copy bandwidth of the MI355X


def torch_rank_mean(rows, lo, hi):
    return torch.sort(torch.stack(rows), dim=0).values[lo:hi].mean(dim=0)


def torch_sqdist(rows):
    x = torch.stack(rows)
    return torch.cdist(x, x) ** 2


def _timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def _inner_count(fn):
    fn()  # first launch: code-object load, library algorithm choice
    torch.cuda.synchronize()
    once = max(_timed(fn, 1), 1e-3)
    return min(max(math.ceil(TARGET_MS / once), 1), 50)


def compare(ours, theirs, reps):
    n_ours, n_theirs = _inner_count(ours), _inner_count(theirs)
    t_ours, t_theirs = [], []
    for _ in range(reps):
        t_ours.append(_timed(ours, n_ours))
        t_theirs.append(_timed(theirs, n_theirs))
    return t_ours, t_theirs


def row(name, k, n, t_ours, t_theirs):
    mo, mt = statistics.median(t_ours), statistics.median(t_theirs)
    gbs = k * n * 4 / (mo * 1e-3) / 1e9
    # faster "by more than the spread": the slowest repetition of ours still
    # beats the fastest repetition of torch
    clear = max(t_ours) < min(t_theirs)
    return (
        f"| {name} | {n:,} | {k} | {mo:.3f} ({min(t_ours):.3f}..{max(t_ours):.3f}) | "
        f"{mt:.3f} ({min(t_theirs):.3f}..{max(t_theirs):.3f}) | {gbs:,.0f} "
        f"({100 * gbs / (PEAK_COPY_TBS * 1e3):.0f}%) | {mt / mo:.2f}x | {'yes' if clear else 'NO'} |"
    )


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7, help="timed repetitions (>= 5)")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    ap.add_argument("--misaligned", action="store_true",
                    help="rows are buf[1:] views (4-byte aligned): times the scalar-load path")
    ap.add_argument("--out", type=str, default=None, help="also write the table to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("robust_agg_micro needs a GPU: timings from a CPU say nothing about the kernels")
    assert F.HAS_EXT, "fl4health_amd._C is not built"

    lines = [
        "| op | n | K | ours ms, median (min..max) | torch ms, median (min..max) | "
        f"ours GB/s of K*n*4 (% of {PEAK_COPY_TBS} TB/s copy) | torch/ours | beyond spread |",
        "|---|---|---|---|---|---|---|---|",
    ]
    print("\n".join(lines), flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for n in args.sizes:
        base = torch.randn(n, device="cuda", generator=gen)
        for k in args.ks:
            # one round's client models: a shared base plus small updates
            pad = 1 if args.misaligned else 0
            bufs = [torch.empty(n + pad, device="cuda") for _ in range(k)]
            rows = [buf[pad:] for buf in bufs]
            for r in rows:
                torch.add(base, torch.randn(n, device="cuda", generator=gen), alpha=1e-2, out=r)
            b = int(0.2 * k)
            lo, hi = (b, k - b) if k - 2 * b >= 1 else (0, k)
            got, want = F.rank_mean_rows(rows, lo, hi), torch_rank_mean(rows, lo, hi)
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), "rank_mean_rows disagrees with torch"
            t = compare(lambda: F.rank_mean_rows(rows, lo, hi), lambda: torch_rank_mean(rows, lo, hi), args.reps)
            lines.append(row(f"rank_mean_rows[{lo}:{hi}]", k, n, *t))
            print(lines[-1], flush=True)
            t = compare(lambda: F.pairwise_sqdist_rows(rows), lambda: torch_sqdist(rows), args.reps)
            lines.append(row("pairwise_sqdist_rows", k, n, *t))
            print(lines[-1], flush=True)
            del rows, bufs
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
