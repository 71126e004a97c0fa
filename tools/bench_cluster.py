"""Library clustering on one MI355X: random unit features, N rows, E components, K centres; alternating A/B windows in one process.

  (a) the assign launch (spmm_centroid_assign, csrc/cluster.hip) against spmm_sim_topk with the roles swapped (the rows as queries, the
      centres as the library, k = 1, one call: its workspace is reported) and against torch.max(f @ c.T, 1) over row chunks; the launch's
      achieved TFLOP/s (2 N K E over its time) against the 157.3 of the exact-f32 MFMA; the same at the other K of --Ks;
  (b) the group + centroids launches against index_add_ + normalise (float atomics: not deterministic, no member lists, no medoids);
  (c) ten k-means iterations (init='random', so the initialisation is not in the window) against the tensor-op form (engine=False);
  (d) pick_diverse(n) against the same loop on torch ops in fp32 (a matrix-vector product, a maximum, an argmin per pick) and, on fewer
      picks, against the float64 tensor-op form (engine=False).

Every timed window is bracketed by device events and repeated `--pairs` times, A and B alternating; the figure is the median window, the
spread (max - min over median) is reported beside it.  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spmm_amd import cluster as C
from spmm_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1_000_000)
ap.add_argument("--E", type=int, default=256)
ap.add_argument("--K", type=int, default=1024)
ap.add_argument("--Ks", type=int, nargs="*", default=[16, 64, 256, 4096], help="further K at which the assign launch is compared")
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--reps", type=int, default=3, help="launches per timed window")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--picks", type=int, default=1000)
ap.add_argument("--picks64", type=int, default=50, help="picks of the float64 tensor-op comparison")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_cluster.py measures on the GPU: no device found (spmm_amd has no CPU / eager fallback)")
dev = torch.device("cuda")
PEAK_F32_MFMA = 157.3


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def alternate(fns, reps):
    """-> ([median ms], [spread], [last output]) of the functions, one warm-up of each, then `pairs` rounds of alternating windows."""
    for fn in fns:
        window(fn, 1)
    times, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(a.pairs):
        for i, fn in enumerate(fns):
            t, outs[i] = window(fn, reps)
            times[i].append(t)
    med = [statistics.median(t) for t in times]
    return med, [(max(t) - min(t)) / m for t, m in zip(times, med)], outs


g = torch.Generator(device=dev).manual_seed(1)
feats = torch.nn.functional.normalize(torch.randn(a.N, a.E, generator=g, device=dev), dim=1)
res = {"device": torch.cuda.get_device_name(0), "N": a.N, "E": a.E, "K": a.K, "pairs": a.pairs, "reps": a.reps}


# ---------------------------------------------------------------------------------------------------------------- (a) assign
def assign_entry(K):
    c = torch.nn.functional.normalize(torch.randn(K, a.E, generator=g, device=dev), dim=1)
    best, idx = torch.empty(a.N, device=dev), torch.empty(a.N, dtype=torch.int32, device=dev)
    s1, i1 = torch.empty(a.N, 1, device=dev), torch.empty(a.N, 1, dtype=torch.int64, device=dev)
    ws = ops.sim_topk_workspace(a.N, K, 1, dev)

    def kernel():
        return ops.centroid_assign(feats, c, best, idx)

    def swapped():
        return ops.sim_topk(feats, c, s1, i1, ws=ws)

    def matmul(rows=65536):
        out_b, out_i = torch.empty(a.N, device=dev), torch.empty(a.N, dtype=torch.int64, device=dev)
        for r0 in range(0, a.N, rows):
            m = torch.max(feats[r0:r0 + rows] @ c.T, 1)
            out_b[r0:r0 + rows], out_i[r0:r0 + rows] = m.values, m.indices
        return out_b, out_i

    med, spread, outs = alternate([kernel, swapped, matmul], a.reps)
    flop = 2.0 * a.N * K * a.E
    return {"centroid_assign_ms": round(med[0], 4), "sim_topk_roles_swapped_ms": round(med[1], 4), "torch_matmul_max_ms": round(med[2], 4),
            "spread": [round(s, 4) for s in spread], "sim_topk_workspace_bytes": int(ws.numel()),
            "speedup_over_sim_topk": round(med[1] / med[0], 3), "speedup_over_torch": round(med[2] / med[0], 3),
            "centroid_assign_TFLOPs": round(flop / (med[0] * 1e-3) / 1e12, 2),
            "share_of_157.3_TF_f32_mfma_peak": round(flop / (med[0] * 1e-3) / 1e12 / PEAK_F32_MFMA, 4),
            "same_bits_as_sim_topk": bool(torch.equal(outs[0][0].view(torch.int32), outs[1][0][:, 0].view(torch.int32))
                                          and torch.equal(outs[0][1].to(torch.int64), outs[1][1][:, 0])),
            "same_index_fraction_vs_torch": round(float((outs[0][1].to(torch.int64) == outs[2][1]).float().mean()), 6),
            "max_abs_best_diff_vs_torch": float((outs[0][0] - outs[2][0]).abs().max())}


res["assign"] = assign_entry(a.K)
res["assign_other_K"] = {f"K{K}": assign_entry(K) for K in a.Ks}

# ---------------------------------------------------------------------------------------------------------------- (b) group + centroids
centres = torch.nn.functional.normalize(torch.randn(a.K, a.E, generator=g, device=dev), dim=1)
best, idx = C.assign(feats, centres)
counts, offsets = torch.empty(a.K, dtype=torch.int32, device=dev), torch.empty(a.K + 1, dtype=torch.int64, device=dev)
members, outside = torch.empty(a.N, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
new, norm, medoid = centres.clone(), torch.empty(a.K, device=dev), torch.empty(a.K, dtype=torch.int32, device=dev)
ws_g, ws_c = ops.cluster_group_workspace(a.N, a.K, dev), ops.cluster_centroids_workspace(a.N, a.K, a.E, dev)
idx64 = idx.to(torch.int64)


def group():
    return ops.cluster_group(idx, a.K, counts, offsets, members, outside, ws=ws_g)


def centroids():
    return ops.cluster_centroids(feats, best, counts, offsets, members, new, norm, medoid, ws=ws_c)


def group_centroids():
    group()
    return centroids()


def index_add():
    return torch.nn.functional.normalize(torch.zeros(a.K, a.E, device=dev).index_add_(0, idx64, feats), dim=1)


med, spread, outs = alternate([group_centroids, index_add, group, centroids], a.reps)
res["update"] = {"group_plus_centroids_ms": round(med[0], 4), "index_add_normalize_ms": round(med[1], 4), "group_ms": round(med[2], 4),
                 "centroids_ms": round(med[3], 4), "spread": [round(s, 4) for s in spread], "speedup_over_index_add": round(med[1] / med[0], 3),
                 "workspace_bytes": [int(ws_g.numel()), int(ws_c.numel())], "max_abs_centre_diff": float((outs[0][0] - outs[1]).abs().max()),
                 "largest_cluster": int(counts.max()), "smallest_cluster": int(counts.min())}

# ---------------------------------------------------------------------------------------------------------------- (c) k-means
med, spread, outs = alternate([lambda: C.kmeans(feats, a.K, iters=a.iters, init="random", seed=0),
                               lambda: C.kmeans(feats, a.K, iters=a.iters, init="random", seed=0, engine=False)], 1)
res["kmeans"] = {"iterations": [outs[0].iterations, outs[1].iterations], "engine_ms": round(med[0], 2), "tensor_ops_float64_ms": round(med[1], 2),
                 "spread": [round(s, 4) for s in spread], "speedup": round(med[1] / med[0], 3),
                 "engine_ms_per_iteration": round(med[0] / max(1, outs[0].iterations), 3),
                 "objective_first_last": [outs[0].objective[0], outs[0].objective[-1]], "reseeded": outs[0].reseeded,
                 "same_assign_fraction": round(float((outs[0].assign == outs[1].assign).float().mean()), 6)}


# ---------------------------------------------------------------------------------------------------------------- (d) pick_diverse
def picks_torch(n, first):
    """The same traversal on torch ops in fp32: per pick a matrix-vector product, a maximum, an argmin."""
    nearest = torch.full((a.N,), float("-inf"), device=dev)
    nxt = torch.tensor([first], device=dev)
    rows = [nxt]
    for j in range(n):
        nearest = torch.maximum(nearest, feats @ feats[nxt[0]])
        nearest[nxt] = float("inf")
        if j + 1 < n:
            nxt = torch.argmin(nearest).view(1)
            rows.append(nxt)
    return torch.cat(rows)


first = C.first_row(a.N, None, 0)
med, spread, outs = alternate([lambda: C.pick_diverse(feats, a.picks, seed=0)[0], lambda: picks_torch(a.picks, first)], 1)
res["pick_diverse"] = {"picks": a.picks, "engine_ms": round(med[0], 2), "torch_fp32_loop_ms": round(med[1], 2), "spread": [round(s, 4) for s in spread],
                       "speedup": round(med[1] / med[0], 3), "engine_ms_per_pick": round(med[0] / a.picks, 4),
                       "same_picks_fraction": round(float((outs[0] == outs[1]).float().mean()), 6)}
med, spread, outs = alternate([lambda: C.pick_diverse(feats, a.picks64, seed=0)[0], lambda: C.pick_diverse(feats, a.picks64, seed=0, engine=False)[0]], 1)
res["pick_diverse_vs_float64_form"] = {"picks": a.picks64, "engine_ms": round(med[0], 2), "tensor_ops_float64_ms": round(med[1], 2),
                                       "spread": [round(s, 4) for s in spread], "speedup": round(med[1] / med[0], 3),
                                       "same_picks": bool(torch.equal(outs[0], outs[1]))}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
