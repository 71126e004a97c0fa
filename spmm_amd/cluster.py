"""Library clustering on the engine's features: which molecules of a library belong together, and which n of them are most unlike
each other?

Everything here works on what `retrieve.MoleculeIndex` holds -- fp32 unit features [N, E] on the device -- and is retrieval's arithmetic
with the roles swapped: every library row asks which of K centres is nearest (csrc/cluster.hip).

  assign        nearest centre of every row: spmm_centroid_assign, the centre list streamed in chunks (any chunking gives the same bits)
  kmeans        spherical k-means: assign -> group (spmm_cluster_group: members of every cluster, ascending) -> centroids
                (spmm_cluster_centroids: fixed-order sums, norms, medoids); empty or cancelled clusters re-seeded from the worst-served rows
  pick_diverse  MaxMin picking = farthest-first traversal: one assign launch per pick with the one new centre and merge = 1
  neighbours / leaders / dedup   threshold clustering (csrc/neighbors.hip), further down: every pair above a threshold, Taylor-Butina and
                first-come leaders on that list -- the number of clusters is a result

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
    """The host mirror of csrc/sim_scan.h's score_key, which defines the order: larger score <-> larger int64 key, -0 = +0, NaN -> 0
    (below -inf's image)."""
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


def _group(idx, K, engine):
    """(counts int32 [K], offsets int64 [K + 1], members int32 [n], -1 past offsets[K]): spmm_cluster_group, or its tensor form."""
    if not (engine and K):
        return _group_tensor(idx, K)
    n, dev = idx.numel(), idx.device
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
    members = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ops.cluster_group(idx, K, counts, offsets, members, torch.empty(1, dtype=torch.int32, device=dev))
    return counts, offsets, members


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
    K, dev = centres.shape[0], f.device
    if engine:
        changed = torch.zeros(1, dtype=torch.int32, device=dev)
        best, idx = assign(f, centres, chunk=chunk, prev=prev, changed=changed)
        counts, offsets, members = _group(idx, K, engine)
        new = centres.clone()
        norm = torch.empty(K, dtype=torch.float32, device=dev)
        medoid = torch.empty(K, dtype=torch.int32, device=dev)
        ops.cluster_centroids(f, best, counts, offsets, members, new, norm, medoid)
    else:
        best, idx = _assign_tensor(f, centres)
        changed = (idx != prev).sum().to(torch.int32).view(1)
        counts, offsets, members = _group(idx, K, engine)
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


# ------------------------------------------------------------------------------------------------------------------ threshold clustering
# Every pair above a threshold, then clusters of a guaranteed radius around real molecules (csrc/neighbors.hip): the number of clusters is
# a result.
#
#   neighbours    the neighbour list of every row: spmm_sim_range twice -- a count pass, a cumsum, an emit pass -- lists ascending, no sort
#   leaders       Taylor-Butina (order="count") or first-come leaders (order="row") on that list: rounds of spmm_leader_round until no row
#                 is open, spmm_leader_finish, clusters numbered in the leaders' priority order, spmm_cluster_group for the members
#   dedup         the rows to keep when near-duplicates are folded into their first occurrence: the leaders under order="row"
#
# Ties of the neighbour count go to the LOWER row (RDKit's Butina.ClusterData gives them to the higher index).
GROUP_MAX_K = 1 << 24       # spmm_cluster_group's limit on the number of clusters
RANGE_CHUNK = 1 << 18       # columns of one spmm_sim_range launch


def _threshold32(threshold) -> float:
    t = float(np.float32(threshold))
    if t != t:
        raise ValueError("the threshold is NaN")
    return t


def _neighbours_tensor(f, t, rows_per_step=2048):
    """(counts, offsets, nbr) from float64 scores by row blocks.  A float64 product may round (i, j) and (j, i) differently, so the relation
    is the union of both directions: symmetric, as the kernel's is by construction."""
    N = f.shape[0]
    f64 = f.double()
    keys = []
    for r0 in range(0, N, rows_per_step):
        S = f64[r0:r0 + rows_per_step] @ f64.T
        i, j = torch.nonzero(S >= t, as_tuple=True)
        i = i + r0
        off = i != j
        keys.append(i[off] * N + j[off])
        keys.append(j[off] * N + i[off])
    key = torch.unique(torch.cat(keys)) if keys else torch.zeros(0, dtype=torch.int64, device=f.device)      # (sorted: row, then column)
    counts = torch.bincount(torch.div(key, max(N, 1), rounding_mode="floor"), minlength=N).to(torch.int32)
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=f.device)
    offsets[1:] = torch.cumsum(counts.to(torch.int64), 0)
    return counts, offsets, (key % max(N, 1)).to(torch.int32)


def _too_many(M, t, max_pairs):
    return ValueError(f"{M} neighbour entries at threshold {t!r} exceed max_pairs={max_pairs} (--max_pairs): raise the threshold, or "
                      f"raise the limit if {4 * M / 2 ** 30:.1f} GiB of list fit in device memory")


def _neighbours(f, t, chunk, max_pairs, engine):
    """-> (counts, offsets, nbr, bad): `bad` is a device flag (the emit pass counted differently from the count pass) not yet read, or None."""
    N = f.shape[0]
    if chunk < 1 or max_pairs < 0:
        raise ValueError(f"neighbours: chunk={chunk} max_pairs={max_pairs}")
    if not engine:
        counts, offsets, nbr = _neighbours_tensor(f, t)
        if nbr.numel() > max_pairs:
            raise _too_many(nbr.numel(), t, max_pairs)
        return counts, offsets, nbr, None
    counts = torch.zeros(N, dtype=torch.int32, device=f.device)
    for c0 in range(0, N, chunk):
        ops.sim_range(f, f[c0:c0 + chunk], t, counts, c0=c0)
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=f.device)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    M = int(offsets[-1])                                                      # the one host read: the size of the list
    if M > max_pairs:
        raise _too_many(M, t, max_pairs)
    nbr = torch.empty(M, dtype=torch.int32, device=f.device)
    again = torch.zeros(N, dtype=torch.int32, device=f.device)
    for c0 in range(0, N, chunk):
        ops.sim_range(f, f[c0:c0 + chunk], t, again, c0=c0, offsets=offsets, nbr=nbr)
    return counts, offsets, nbr, (again != counts).any()


def _refuse_emit_mismatch(bad):
    """`bad`: _neighbours' flag once it has been read on the host."""
    if bad:
        raise RuntimeError("neighbours: the emit pass counted other neighbours than the count pass")


@torch.no_grad()
def neighbours(feats, threshold: float, chunk: int = RANGE_CHUNK, max_pairs: int = 1 << 30, engine: bool = True):
    """Every row's neighbours above a threshold -> (counts int32 [N], offsets int64 [N + 1], nbr int32 [M]): the neighbours of row i -- the
    rows j != i with cosine(i, j) >= threshold (rounded to fp32) -- are nbr[offsets[i]:offsets[i + 1]], ascending.  The relation is exactly
    symmetric, an exact copy of a row is its neighbour, a NaN row has none.  The column side is streamed `chunk` rows at a time (any
    chunking gives the same bytes).  M, read once between the two passes, is refused above `max_pairs` before the list is allocated."""
    f = _feats(feats)
    counts, offsets, nbr, bad = _neighbours(f, _threshold32(threshold), chunk, max_pairs, engine)
    _refuse_emit_mismatch(bad is not None and bool(bad))
    return counts, offsets, nbr


@dataclass
class LeaderClustering:
    """The result of `leaders` over N rows: K clusters, each a leader (a real row) and the rows it claimed, every member within the
    threshold of its leader, no two leaders within it.  Cluster 0 is the first leader in priority order (order="count": the most populated
    neighbourhood).  The rows of cluster c are members[offsets[c]:offsets[c + 1]], ascending."""
    leader: torch.Tensor           # int32 [N]: the row's leader (itself for a leader)
    cluster: torch.Tensor          # int32 [N]
    leaders: torch.Tensor          # int64 [K]: the leader rows, in cluster order
    counts: torch.Tensor           # int32 [K]
    offsets: torch.Tensor          # int64 [K + 1]
    members: torch.Tensor          # int32 [N]
    n_neighbours: torch.Tensor     # int32 [N]
    cosine_to_leader: Optional[torch.Tensor]   # fp32 [N], 1.0 for a leader (None when only a list was given)
    rounds: int                    # rounds of the parallel rule until no row was open
    threshold: Optional[float]
    order: str
    pairs: int                     # entries of the neighbour list (every pair twice)


def _leaders_sequential(counts, offsets, nbr, by_count):
    """The sequential algorithm in numpy -> (leader int64 [N], rounds): visit the rows in priority order; a row not yet claimed becomes a
    leader and claims its unclaimed neighbours.  `rounds` is what the parallel rule needs, from the same walk: a leader is decided one
    round after the last of its higher-priority neighbours, a member one round after the first of its higher-priority leaders."""
    cnt, off, nb = counts.cpu().numpy().astype(np.int64), offsets.cpu().numpy(), nbr.cpu().numpy().astype(np.int64)
    N = cnt.shape[0]
    order = np.lexsort((np.arange(N), -cnt)) if by_count else np.arange(N)
    rank = np.empty(N, dtype=np.int64)
    rank[order] = np.arange(N)
    leader = np.full(N, -1, dtype=np.int64)
    decided = np.zeros(N, dtype=np.int64)
    for i in order.tolist():
        mine = nb[off[i]:off[i + 1]]
        higher = mine[rank[mine] < rank[i]]
        if leader[i] < 0:
            leader[i] = i
            decided[i] = 1 + (decided[higher].max() if higher.size else 0)
            free = mine[leader[mine] < 0]
            leader[free] = i
        else:
            led = higher[leader[higher] == higher]
            decided[i] = 1 + (decided[led].min() if led.size else 0)      # (no such leader: the list was not symmetric)
    return leader, int(decided.max()) if N else 0


def _run_rounds(counts, offsets, nbr, by_count, sync_every, bad):
    """Rounds of spmm_leader_round until one leaves no row open -> (state, rounds).  The open counts are read every `sync_every` rounds;
    a round past the last one copies the state, so neither depends on sync_every.  `bad` (neighbours' device flag) rides on the first read."""
    N, dev = counts.numel(), counts.device
    state, other = torch.zeros(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    rounds = 0
    while True:
        opened = torch.zeros(sync_every + 1, dtype=torch.int32, device=dev)
        for r in range(sync_every):
            ops.leader_round(counts, offsets, nbr, state, other, opened[r:r + 1], by_count=by_count)
            state, other = other, state
        if bad is not None:
            opened[sync_every] = bad.to(torch.int32)
        host = opened.tolist()                                               # the one host read of these rounds
        _refuse_emit_mismatch(host[sync_every])                              # (0 when no flag rode along)
        bad = None
        for r in range(sync_every):
            if host[r] == 0:
                return state, rounds + r + 1
        rounds += sync_every


@torch.no_grad()
def leaders(feats_or_csr, threshold: Optional[float] = None, order: str = "count", sync_every: int = 4, chunk: int = RANGE_CHUNK,
            max_pairs: int = 1 << 30, engine: bool = True) -> LeaderClustering:
    """Threshold clustering of the rows: Taylor-Butina (order="count": the row with the most neighbours leads first, equal counts to the
    lower row) or first-come leaders (order="row").  feats_or_csr: a MoleculeIndex / [N, E] features with a `threshold`, or a symmetric
    neighbour list (counts, offsets, nbr) as `neighbours` returns it.  The parallel rule of spmm_leader_round gives the sequential
    algorithm's result; its worst case is one round per row (a path under order="row"), a similarity graph takes a handful."""
    if order not in ("count", "row"):
        raise ValueError(f"leaders: order={order!r}: 'count' or 'row'")
    if sync_every < 1:
        raise ValueError(f"leaders: sync_every={sync_every}")
    by_count = order == "count"
    f, bad, t = None, None, None
    if isinstance(feats_or_csr, (tuple, list)):
        n_nb, offsets, nbr = feats_or_csr
        n_nb, offsets, nbr = n_nb.to(torch.int32).contiguous(), offsets.to(torch.int64).contiguous(), nbr.to(torch.int32).contiguous()
    else:
        if threshold is None:
            raise ValueError("leaders: features need a threshold")
        f, t = _feats(feats_or_csr), _threshold32(threshold)
        n_nb, offsets, nbr, bad = _neighbours(f, t, chunk, max_pairs, engine)
    N, dev = n_nb.numel(), n_nb.device
    if engine:
        if N:
            state, rounds = _run_rounds(n_nb, offsets, nbr, by_count, sync_every, bad)
        else:
            state, rounds = torch.zeros(0, dtype=torch.int32, device=dev), 0
        leader = torch.empty(N, dtype=torch.int32, device=dev)
        ops.leader_finish(n_nb, offsets, nbr, state, leader, by_count=by_count)
    else:
        lead, rounds = _leaders_sequential(n_nb, offsets, nbr, by_count)
        leader = torch.from_numpy(lead).to(dev).to(torch.int32)
    ar = torch.arange(N, device=dev)
    rows = torch.nonzero(leader.to(torch.int64) == ar).flatten()
    if by_count:                                                              # a sort over the leaders only: more neighbours first, then the lower row
        rows = rows[torch.sort(rows - n_nb[rows].to(torch.int64) * N).indices]
    K = rows.numel()
    if K > GROUP_MAX_K:
        raise ValueError(f"leaders: {K} clusters exceed spmm_cluster_group's limit of 2^24 = {GROUP_MAX_K}: lower the threshold")
    number = torch.full((N,), -1, dtype=torch.int32, device=dev)
    number[rows] = torch.arange(K, dtype=torch.int32, device=dev)
    lead64 = leader.to(torch.int64)
    cluster = torch.where(lead64 >= 0, number[lead64.clamp_min(0)], torch.full_like(number, -1)) if N else number
    counts, offs, members = _group(cluster, K, engine)
    cos = None
    if f is not None:
        cos = (f * f.index_select(0, lead64.clamp_min(0))).sum(1)
        cos = torch.where(lead64 == ar, torch.ones_like(cos), cos)
    return LeaderClustering(leader=leader, cluster=cluster, leaders=rows, counts=counts, offsets=offs, members=members, n_neighbours=n_nb,
                            cosine_to_leader=cos, rounds=rounds, threshold=t, order=order, pairs=int(nbr.numel()))


@torch.no_grad()
def dedup(feats, threshold: float, engine: bool = True, max_pairs: int = 1 << 30) -> torch.Tensor:
    """keep bool [N]: False for a row within `threshold` of an earlier kept row -- the leaders under order="row", so the first occurrence of
    every set of near-duplicates stays and `leaders(..., order="row").leader` names the row each dropped one was folded into."""
    res = leaders(feats, threshold, order="row", engine=engine, max_pairs=max_pairs)
    return res.leader.to(torch.int64) == torch.arange(res.leader.numel(), device=res.leader.device)
