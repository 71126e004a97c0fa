"""Library clustering on the engine's features: which molecules of a library belong together, and which n of them are most unlike
each other?

Everything here works on what `retrieve.MoleculeIndex` holds -- fp32 unit features [N, E] on the device -- and is retrieval's arithmetic
with the roles swapped: every library row asks which of K centres is nearest (csrc/cluster.hip).

  assign        nearest centre of every row: spmm_centroid_assign, the centre list streamed in chunks (any chunking gives the same bits)
  kmeans        spherical k-means: assign -> group (spmm_cluster_group: members of every cluster, ascending) -> centroids
                (spmm_cluster_centroids: fixed-order sums, norms, medoids); empty or cancelled clusters re-seeded from the worst-served rows
  pick_diverse  MaxMin picking = farthest-first traversal: one assign launch per pick with the one new centre and merge = 1

Deterministic: no floating-point atomics, every sum in an order fixed by the data; two runs agree bit for bit.  Inference only.
`engine=False` is the tensor-library form of the same rules with float64 scores (runs on CPU tensors): the yard-stick of the tests and of
tools/bench_cluster.py, not a fallback -- the default path is HIP and fails without the library."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops

NORM_GUARD = 1e-12          # spmm_cluster_centroids writes a centre only when the length of the members' sum reaches this
MAX_K = 65536               # clusters the driver accepts


def _feats(index_or_feats) -> torch.Tensor:
    f = getattr(index_or_feats, "feats", index_or_feats)
    if not isinstance(f, torch.Tensor) or f.dim() != 2:
        raise TypeError("clustering takes a MoleculeIndex or an [N, E] tensor")
    f = f.to(torch.float32)
    if f.stride(1) != 1 or f.stride(0) % 4 or f.data_ptr() % 16:
        f = f.contiguous()
    return f


def _score_key(best: torch.Tensor) -> torch.Tensor:
    """spmm_sim_topk's order of scores as an int64 key: larger score <-> larger key, -0 = +0, NaN -> 0 (below -inf's image)."""
    b = best.to(torch.float32) + 0.0
    u = b.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)
    return torch.where(torch.isnan(b), torch.zeros_like(key), key)


def first_row(N: int, first: Optional[int] = None, seed: int = 0) -> int:
    """The first pick of a farthest-first traversal: `first`, or a row drawn from `seed`."""
    return int(first) if first is not None else int(np.random.default_rng(seed).integers(N))


# ------------------------------------------------------------------------------------------------------------------ tensor-op forms
def _assign_tensor(f, c, rows_per_step=4096):
    """(best fp32 [n], assign int32 [n]) from float64 scores, in the kernel's candidate order; forms [rows_per_step, K] at a time."""
    n, K = f.shape[0], c.shape[0]
    c64 = c.double()
    ar = torch.arange(K, device=f.device)
    best = torch.empty(n, dtype=torch.float32, device=f.device)
    idx = torch.empty(n, dtype=torch.int32, device=f.device)
    for r0 in range(0, n, rows_per_step):
        S = f[r0:r0 + rows_per_step].double() @ c64.T
        num = ~torch.isnan(S)
        m = torch.where(num, S, torch.full_like(S, float("-inf"))).max(1).values
        i_num = torch.where(num & (S == m[:, None]), ar, K).min(1).values
        i_nan = torch.where(~num, ar, K).min(1).values
        has = num.any(1)
        best[r0:r0 + rows_per_step] = torch.where(has, m + 0.0, torch.full_like(m, float("nan"))).float()
        idx[r0:r0 + rows_per_step] = torch.where(has, i_num, i_nan).to(torch.int32)
    return best, idx


def _merge_tensor(best, idx, nb, ni):
    """The better of two candidates per row (state first): larger score, then lower index; NaN below numbers; index < 0 is empty."""
    ka, kb = _score_key(best), _score_key(nb)
    take = (ni >= 0) & ((idx < 0) | (kb > ka) | ((kb == ka) & (ni < idx)))
    return torch.where(take, nb, best), torch.where(take, ni, idx)


def _group_tensor(idx, K):
    n = idx.numel()
    a = idx.to(torch.int64)
    valid = (a >= 0) & (a < K)
    counts = torch.bincount(a[valid], minlength=K).to(torch.int32)
    offsets = torch.zeros(K + 1, dtype=torch.int64, device=idx.device)
    offsets[1:] = torch.cumsum(counts.to(torch.int64), 0)
    order = torch.sort(torch.where(valid, a, torch.full_like(a, K)), stable=True).indices
    members = torch.full((n,), -1, dtype=torch.int32, device=idx.device)
    nv = int(valid.sum())
    members[:nv] = order[:nv].to(torch.int32)
    return counts, offsets, members


def _centroids_tensor(f, best, idx, counts, offsets, members, centres):
    K, E = centres.shape
    a = idx.to(torch.int64)
    valid = (a >= 0) & (a < K)
    sums = torch.zeros(K, E, dtype=torch.float64, device=f.device).index_add_(0, a[valid], f[valid].double())
    norm = sums.norm(dim=1)
    ok = (counts > 0) & (norm >= NORM_GUARD)
    new = torch.where(ok[:, None], (sums / norm.clamp_min(1e-300)[:, None]).float(), centres)
    # medoid: within a cluster, the largest best, ties to the lowest row -- two stable sorts
    rows = torch.nonzero(valid).flatten()
    by_best = rows[torch.sort(_score_key(best[rows]), descending=True, stable=True).indices]
    by_cluster = by_best[torch.sort(a[by_best], stable=True).indices]
    medoid = torch.full((K,), -1, dtype=torch.int32, device=f.device)
    has = counts > 0
    medoid[has] = by_cluster[offsets[:-1][has]].to(torch.int32)
    return new, norm.float(), medoid


# ------------------------------------------------------------------------------------------------------------------ assign
@torch.no_grad()
def assign(feats, centres: torch.Tensor, chunk: int = 4096, engine: bool = True, prev=None, changed=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Nearest centre of every row -> (best fp32 [N], assign int32 [N]): the largest cosine and its centre, equal scores to the lowest
    centre index.  The centre list is streamed `chunk` centres at a time (any chunking gives the same bits).  prev / changed (engine only):
    changed += the rows whose assignment differs from prev."""
    f = _feats(feats)
    c = _feats(centres.to(f.device))
    if c.shape[1] != f.shape[1] or c.shape[0] < 1 or chunk < 1:
        raise ValueError(f"centres {tuple(c.shape)} do not match the features {tuple(f.shape)} (chunk={chunk})")
    if not engine:
        return _assign_tensor(f, c)
    N, K = f.shape[0], c.shape[0]
    best = torch.empty(N, dtype=torch.float32, device=f.device)
    idx = torch.empty(N, dtype=torch.int32, device=f.device)
    for c0 in range(0, K, chunk):
        last = c0 + chunk >= K
        ops.centroid_assign(f, c[c0:c0 + chunk], best, idx, c0=c0, merge=c0 > 0, prev=prev if last else None, changed=changed if last else None)
    return best, idx


# ------------------------------------------------------------------------------------------------------------------ pick_diverse
@torch.no_grad()
def pick_diverse(feats, n: int, first: Optional[int] = None, seed: int = 0, engine: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """MaxMin picking (farthest-first traversal) -> (rows int64 [n], similarity fp32 [n]): pick 0 is `first` (or a row drawn from `seed`),
    pick j + 1 the row least similar to its nearest earlier pick -- NaN rows excluded, equal values to the lowest row, a row never twice.
    similarity[j] = pick j's largest cosine to the earlier picks (-inf for pick 0).  One spmm_centroid_assign launch per pick (the one new
    centre, merge = 1: the running best is every row's similarity to its nearest pick), a device argmin and a device row gather; no host
    read inside the loop."""
    f = _feats(feats)
    N = f.shape[0]
    if not 1 <= n <= N:
        raise ValueError(f"pick_diverse: n={n} must be in [1, {N}]")
    r0 = first_row(N, first, seed)
    if not 0 <= r0 < N:
        raise ValueError(f"pick_diverse: first={r0} is not a row of the library")
    dev = f.device
    best = torch.full((N,), float("-inf"), dtype=torch.float32, device=dev)
    idx = torch.full((N,), -1, dtype=torch.int32, device=dev)
    picked = torch.zeros(N, dtype=torch.bool, device=dev)
    ar = torch.arange(N, device=dev)
    nxt = torch.tensor([r0], dtype=torch.int64, device=dev)
    rows, sims = [nxt], [torch.full((1,), float("-inf"), dtype=torch.float32, device=dev)]
    big = torch.finfo(torch.float32).max
    for j in range(n):
        picked[nxt] = True
        centre = f.index_select(0, nxt)
        if engine:
            ops.centroid_assign(f, centre, best, idx, c0=j, merge=j > 0)
        else:
            nb, ni = _assign_tensor(f, centre)
            best, idx = (nb, ni + j) if j == 0 else _merge_tensor(best, idx, nb, ni + j)
        if j + 1 == n:
            break
        val = torch.where(torch.isnan(best), torch.full_like(best, big), best)
        val = torch.where(picked, torch.full_like(best, float("inf")), val)
        nxt = torch.where(val == val.min(), ar, N).min().view(1)             # (the lowest row among equal minima)
        rows.append(nxt)
        sims.append(best.index_select(0, nxt))
    return torch.cat(rows), torch.cat(sims)


# ------------------------------------------------------------------------------------------------------------------ k-means
@dataclass
class Clustering:
    """The result of `kmeans` over N rows and k clusters.  `assign` / `best` are every row's nearest centre and its cosine under the centres
    the last iteration STARTED from; `centres` are the centres it ended with (equal once `changed` reached 0 and nothing was re-seeded).
    The rows of cluster c are members[offsets[c]:offsets[c + 1]], ascending (entries past offsets[k] are -1); medoid[c] is its member nearest
    the centre (-1 for an empty cluster)."""
    centres: torch.Tensor          # fp32 [k, E], unit rows
    assign: torch.Tensor           # int32 [N]
    best: torch.Tensor             # fp32 [N]
    counts: torch.Tensor           # int32 [k]
    offsets: torch.Tensor          # int64 [k + 1]
    members: torch.Tensor          # int32 [N]
    medoid: torch.Tensor           # int32 [k]
    objective: List[float]         # per iteration: the sum of best over the rows
    iterations: int
    reseeded: int                  # clusters given a new centre because they were empty or their sum cancelled, over all iterations
    changed: int                   # rows that changed cluster in the last iteration (0: converged)


def _reseed(f, best, bad, centres):
    """Centres of the bad clusters from the worst-served rows: the e-th bad cluster (ascending) takes the row with the e-th lowest best
    (spmm_sim_topk's order, ties to the lowest row).  Tensor ops of fixed shapes: no host read."""
    N, K = f.shape[0], centres.shape[0]
    key = _score_key(best) * N + torch.arange(N, device=f.device)            # (distinct keys: the sort needs no stability)
    order = torch.sort(key).indices[:min(K, N)]
    rank = (torch.cumsum(bad.to(torch.int64), 0) - 1).clamp_(0, order.numel() - 1)
    return torch.where(bad[:, None], f.index_select(0, order.index_select(0, rank)), centres)


def _iteration(f, centres, prev, chunk, engine):
    """assign -> group -> centroids -> re-seed, all enqueued: -> dict of device tensors (nothing read on the host)."""
    N, E = f.shape
    K, dev = centres.shape[0], f.device
    if engine:
        changed = torch.zeros(1, dtype=torch.int32, device=dev)
        best, idx = assign(f, centres, chunk=chunk, prev=prev, changed=changed)
        counts = torch.empty(K, dtype=torch.int32, device=dev)
        offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
        members = torch.full((N,), -1, dtype=torch.int32, device=dev)
        ops.cluster_group(idx, K, counts, offsets, members, torch.empty(1, dtype=torch.int32, device=dev))
        new = centres.clone()
        norm = torch.empty(K, dtype=torch.float32, device=dev)
        medoid = torch.empty(K, dtype=torch.int32, device=dev)
        ops.cluster_centroids(f, best, counts, offsets, members, new, norm, medoid)
    else:
        best, idx = _assign_tensor(f, centres)
        changed = (idx != prev).sum().to(torch.int32).view(1)
        counts, offsets, members = _group_tensor(idx, K)
        new, norm, medoid = _centroids_tensor(f, best, idx, counts, offsets, members, centres)
    bad = (counts == 0) | ~(norm >= NORM_GUARD)
    new = _reseed(f, best, bad, new)
    stats = torch.stack([changed.double().view(()), bad.sum().double(), best.double().sum()])
    return dict(centres=new, assign=idx, best=best, counts=counts, offsets=offsets, members=members, medoid=medoid, stats=stats)


@torch.no_grad()
def kmeans(feats, k: int, iters: int = 20, init: str = "farthest", seed: int = 0, sync_every: int = 4, chunk: int = 4096,
           engine: bool = True) -> Clustering:
    """Spherical k-means of the rows into k clusters.  init: 'farthest' = the rows `pick_diverse(feats, k, seed=seed)` picks, 'random' = k
    distinct rows drawn from `seed`.  Each iteration is three entry points (assign, group, centroids) and a re-seed of the clusters that
    came out empty or whose members' sum cancelled; the loop ends at the first iteration in which no row changed cluster, or at `iters`.
    The device's change count is read every `sync_every` iterations only; the iterations enqueued past the converged one are discarded,
    so the result does not depend on `sync_every`."""
    f = _feats(feats)
    N = f.shape[0]
    if not 1 <= k <= N:
        raise ValueError(f"kmeans: k={k} must be in [1, {N}]")
    if iters < 1 or sync_every < 1:
        raise ValueError(f"kmeans: iters={iters} sync_every={sync_every}")
    if init == "farthest":
        rows = pick_diverse(f, k, seed=seed, engine=engine)[0]
    elif init == "random":
        rows = torch.from_numpy(np.random.default_rng(seed).choice(N, size=k, replace=False).astype(np.int64)).to(f.device)
    else:
        raise ValueError(f"kmeans: init={init!r}: 'farthest' or 'random'")
    centres = f.index_select(0, rows).contiguous()
    prev = torch.full((N,), -1, dtype=torch.int32, device=f.device)
    done: List[dict] = []
    pending: List[dict] = []
    converged = False
    for it in range(iters):
        step = _iteration(f, centres, prev, chunk, engine)
        pending.append(step)
        centres, prev = step["centres"], step["assign"]
        if len(pending) == sync_every or it + 1 == iters:
            stats = torch.stack([s["stats"] for s in pending]).cpu()          # the one host read of these iterations
            for s, row in zip(pending, stats.tolist()):
                s["stats"] = row
                done.append(s)
                if row[0] == 0:
                    converged = True
                    break
            pending = []
            if converged:
                break
    last = done[-1]
    return Clustering(centres=last["centres"], assign=last["assign"], best=last["best"], counts=last["counts"], offsets=last["offsets"],
                      members=last["members"], medoid=last["medoid"], objective=[s["stats"][2] for s in done], iterations=len(done),
                      reseeded=int(sum(s["stats"][1] for s in done)), changed=int(last["stats"][0]))
