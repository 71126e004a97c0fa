"""Threshold clustering on one MI355X: seeded planted-mixture unit features (groups of --group rows around random unit centres, so that
neighbourhoods are not empty), N rows, E components, the threshold chosen from a sample of rows for a mean degree near --degree;
alternating windows in one process.  Per N of --Ns:

  (a) the count pass and the emit pass of spmm_sim_range (csrc/neighbors.hip) against the chunked tensor-library route
      (f[rows] @ f.T >= t).sum(1) / .nonzero(); each pass's achieved TFLOP/s (2 N^2 E over its time) against the 157.3 of the exact-f32
      MFMA -- a whole-launch rate, not a kernel trace;
  (b) the leader rounds + finish on the list against the sequential numpy pass over the same list (spmm_amd.cluster's engine=False walk,
      the list already on the host);
  (c) the whole leaders() call (both passes, the cumsum, the rounds, finish, numbering, grouping).

Every window is a host clock around work that ends in a device synchronise, repeated `--pairs` times, the routes alternating (the host
walk `--host_pairs` times); the figure is the median window, the spread (max - min over median) is reported beside it.  Prints one JSON
line and, with --out, writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spmm_amd import cluster as C
from spmm_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--Ns", type=int, nargs="*", default=[100_000, 1_000_000])
ap.add_argument("--E", type=int, default=256)
ap.add_argument("--group", type=int, default=64, help="rows of a planted group")
ap.add_argument("--noise", type=float, default=0.5, help="length of a row's noise relative to its centre (within-group cosine 1 / (1 + noise^2))")
ap.add_argument("--degree", type=float, default=50.0, help="mean degree the threshold is chosen for")
ap.add_argument("--sample", type=int, default=512, help="rows whose scores choose the threshold")
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--host_pairs", type=int, default=7, help="windows of the sequential numpy walk")
ap.add_argument("--order", default="count", choices=("count", "row"))
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_butina.py measures on the GPU: no device found (spmm_amd has no CPU / eager fallback)")
dev = torch.device("cuda")
PEAK_F32_MFMA = 157.3


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(fns, pairs):
    """-> ([median ms], [spread], [last output]) of the functions, one warm-up of each, then `pairs` rounds of alternating windows."""
    for fn in fns:
        window(fn)
    times, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(pairs):
        for i, fn in enumerate(fns):
            t, outs[i] = window(fn)
            times[i].append(t)
    med = [statistics.median(t) for t in times]
    return med, [(max(t) - min(t)) / m for t, m in zip(times, med)], outs


def features(N):
    g = torch.Generator(device=dev).manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn((N + a.group - 1) // a.group, a.E, generator=g, device=dev), dim=1)
    label = torch.randperm(N, generator=g, device=dev) // a.group
    noise = torch.randn(N, a.E, generator=g, device=dev) * (a.noise / a.E ** 0.5)
    return torch.nn.functional.normalize(centres[label] + noise, dim=1)


def choose_threshold(f):
    """The score such that the sampled rows have --degree neighbours on average (their own score left out)."""
    N = f.shape[0]
    rows = torch.arange(0, N, max(1, N // a.sample), device=dev)[:a.sample]
    S = f[rows] @ f.T
    S[torch.arange(rows.numel(), device=dev), rows] = -2.0
    k = int(a.degree * rows.numel())
    per_row = min(N, max(4 * int(a.degree), 2 * a.group))                    # (no sampled row has more scores than this above the threshold)
    top = torch.sort(torch.topk(S, per_row, dim=1).values.flatten(), descending=True).values
    return float((top[k - 1] + top[k]) / 2)


def entry(N):
    f = features(N)
    t = C._threshold32(choose_threshold(f))
    step = max(256, (1 << 29) // N)                                          # rows of one [rows, N] fp32 score block: 2 GiB
    flop = 2.0 * N * N * a.E
    counts = torch.zeros(N, dtype=torch.int32, device=dev)
    ops.sim_range(f, f, t, counts)
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    M = int(offsets[-1])
    nbr = torch.empty(M, dtype=torch.int32, device=dev)
    state = torch.empty(N, dtype=torch.int32, device=dev)

    def count_kernel():
        state.zero_()
        return ops.sim_range(f, f, t, state)

    def emit_kernel():
        state.zero_()
        ops.sim_range(f, f, t, state, offsets=offsets, nbr=nbr)
        return nbr

    def count_torch():
        out = torch.empty(N, dtype=torch.int64, device=dev)
        for r0 in range(0, N, step):
            out[r0:r0 + step] = (f[r0:r0 + step] @ f.T >= t).sum(1)
        return out - 1                                                        # (a unit row's own score is above any threshold below 1)

    def emit_torch():
        pieces = []
        for r0 in range(0, N, step):
            i, j = (f[r0:r0 + step] @ f.T >= t).nonzero(as_tuple=True)
            pieces.append(j[j != i + r0].to(torch.int32))
        return torch.cat(pieces)

    print(f"# N={N}: threshold {t!r}, M={M}", file=sys.stderr, flush=True)
    med, spread, outs = alternate([count_kernel, emit_kernel, count_torch, emit_torch], a.pairs)
    print(f"# N={N}: passes {[round(m, 2) for m in med]} ms", file=sys.stderr, flush=True)
    res = {"N": N, "threshold": t, "M": M, "mean_degree": round(M / N, 3), "max_degree": int(counts.max()),
           "list_bytes": 4 * M, "torch_rows_per_block": step,
           "count_pass_ms": round(med[0], 3), "emit_pass_ms": round(med[1], 3), "torch_count_ms": round(med[2], 3),
           "torch_nonzero_ms": round(med[3], 3), "spread": [round(s, 4) for s in spread],
           "count_pass_TFLOPs": round(flop / (med[0] * 1e-3) / 1e12, 2), "emit_pass_TFLOPs": round(flop / (med[1] * 1e-3) / 1e12, 2),
           "count_share_of_157.3_TF_f32_mfma_peak": round(flop / (med[0] * 1e-3) / 1e12 / PEAK_F32_MFMA, 4),
           "emit_share_of_157.3_TF_f32_mfma_peak": round(flop / (med[1] * 1e-3) / 1e12 / PEAK_F32_MFMA, 4),
           "count_speedup_over_torch": round(med[2] / med[0], 3), "emit_speedup_over_torch": round(med[3] / med[1], 3),
           "emit_counts_equal_count_pass": bool(torch.equal(state, counts)),
           "counts_equal_fraction_vs_torch": round(float((outs[0].to(torch.int64) == outs[2]).float().mean()), 6),
           "list_entries_torch": int(outs[3].numel())}

    # (b) the rounds and finish on the list, against the sequential walk on the host
    by_count = a.order == "count"
    leader = torch.empty(N, dtype=torch.int32, device=dev)
    rounds = [0]

    def rounds_engine():
        st, rounds[0] = C._run_rounds(counts, offsets, nbr, by_count, 4, None)
        return ops.leader_finish(counts, offsets, nbr, st, leader, by_count=by_count)

    med, spread, outs = alternate([rounds_engine], a.pairs)
    print(f"# N={N}: rounds {rounds[0]}, {med[0]:.2f} ms", file=sys.stderr, flush=True)
    host = (counts.cpu(), offsets.cpu(), nbr.cpu())
    walk = []
    for _ in range(max(1, a.host_pairs)):
        t0 = time.perf_counter()
        seq, seq_rounds = C._leaders_sequential(*host, by_count)
        walk.append((time.perf_counter() - t0) * 1e3)
        print(f"# N={N}: sequential walk {walk[-1]:.0f} ms", file=sys.stderr, flush=True)
    wmed = statistics.median(walk)
    res["leaders_on_the_list"] = {"order": a.order, "rounds": rounds[0], "rounds_plus_finish_ms": round(med[0], 3), "spread": round(spread[0], 4),
                                  "sequential_numpy_ms": round(wmed, 2), "sequential_windows": len(walk),
                                  "sequential_spread": round((max(walk) - min(walk)) / wmed, 4), "speedup": round(wmed / med[0], 2),
                                  "same_leaders": bool((torch.from_numpy(seq).to(dev) == outs[0].to(torch.int64)).all()),
                                  "same_rounds": seq_rounds == rounds[0]}
    # (c) the whole call
    med, spread, outs = alternate([lambda: C.leaders(f, t, order=a.order)], a.pairs)
    sizes = outs[0].counts
    res["leaders_call"] = {"ms": round(med[0], 2), "spread": round(spread[0], 4), "clusters": int(sizes.numel()),
                           "singletons": int((sizes == 1).sum()), "largest_cluster": int(sizes.max()), "rounds": outs[0].rounds,
                           "share_of_the_two_passes": round((res["count_pass_ms"] + res["emit_pass_ms"]) / med[0], 4)}
    return res


out = {"device": torch.cuda.get_device_name(0), "E": a.E, "group": a.group, "noise": a.noise, "target_degree": a.degree, "pairs": a.pairs,
       "runs": [entry(N) for N in a.Ns]}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
