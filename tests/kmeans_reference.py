"""TEST INFRASTRUCTURE (never imported by spmm_amd/): library clustering restated in float64 numpy, with no torch kernels -- the nearest
centre of every row, the members of every cluster, the centres / norms / medoids, the spherical k-means loop and farthest-first
traversal as spmm_amd/cluster.py and csrc/cluster.hip specify them, one plain loop per rule.

Order of candidates (spmm_sim_topk's): larger score first, equal scores by ascending centre index, NaN below every number, -0 = +0
(returned as +0), the empty slot (-inf, -1) below everything.

DELTA[E] is the tolerance of an fp32 score against float64 and CENTROID_TOL that of a centre / norm component: four times the largest
deviation the kernels showed over the cases of tests/test_cluster_kernels_gpu.py on an MI355X (profiles/cluster_tol.txt holds both
numbers), each under its cap: DELTA[E] <= E 2^-23, twice the first-order bound of an E-term fmaf chain on unit vectors; a centre's error at
most that of a plain sequential fp32 sum, `centroid_cap`."""
from __future__ import annotations

import numpy as np

DELTA = {64: 4 * 1.626e-7, 256: 4 * 1.612e-7}             # measured 1.626e-07 (E = 64, n = 256, K = 65) and 1.612e-07 (E = 256, n = 255, K = 65)
CENTROID_TOL = 4 * 8.335e-8                               # measured 8.335e-08 (E = 100)
DELTA_CAP = {E: E * 2.0 ** -23 for E in (64, 128, 192, 256, 320, 384, 448, 512)}
GUARD = 1e-12

NEG_INF = float("-inf")


# ------------------------------------------------------------------------------------------------------------------ order
def better(sa, ia, sb, ib) -> bool:
    """Is candidate (sa, ia) strictly better than (sb, ib)?  An index < 0 is the empty slot."""
    if ia < 0:
        return False
    if ib < 0:
        return True
    na, nb = sa != sa, sb != sb
    if na or nb:
        return (nb and not na) or (na and nb and ia < ib)
    return sa > sb or (sa == sb and ia < ib)


def scores64(f, c):
    """float64 scores [n, K]; every entry is the same sum over E whatever n and K are (a BLAS product rounds an entry differently in
    differently shaped calls, which would make exact copies of a centre score differently across chunkings)."""
    f64, c64 = np.asarray(f, dtype=np.float64), np.asarray(c, dtype=np.float64)
    out = np.empty((f64.shape[0], c64.shape[0]))
    for r0 in range(0, f64.shape[0], 64):
        out[r0:r0 + 64] = (f64[r0:r0 + 64, None, :] * c64[None, :, :]).sum(-1)
    return out


# ------------------------------------------------------------------------------------------------------------------ assign
def assign(f, c, c0=0, state=None, S=None):
    """-> (best float64 [n], assign int64 [n], second float64 [n]): the best candidate of every row among centres c0 .. c0 + Kc - 1 and the
    state (best, assign) if given; `second` is the best score among the OTHER candidates (-inf if none): best - second is the margin of
    the decision."""
    S = scores64(f, c) if S is None else S
    n, Kc = S.shape
    best = np.full(n, NEG_INF)
    idx = np.full(n, -1, dtype=np.int64)
    second = np.full(n, NEG_INF)
    for i in range(n):
        cands = [(S[i, j], c0 + j) for j in range(Kc)]
        if state is not None and state[1][i] >= 0:
            cands.append((float(state[0][i]), int(state[1][i])))
        bs, bi = NEG_INF, -1
        for s, j in cands:
            if better(s, j, bs, bi):
                bs, bi = s, j
        rest = [s for s, j in cands if j != bi and s == s]
        best[i] = bs + 0.0 if bs == bs else bs                 # (-0 + 0 = +0)
        idx[i] = bi
        second[i] = max(rest) if rest else NEG_INF
    return best, idx, second


# ------------------------------------------------------------------------------------------------------------------ group
def group(assign_, K):
    """-> (counts int64 [K], offsets int64 [K + 1], members int64 [in a cluster], outside): members of cluster c ascending."""
    lists = [[] for _ in range(K)]
    outside = 0
    for i, a in enumerate(np.asarray(assign_).tolist()):
        if 0 <= a < K:
            lists[a].append(i)
        else:
            outside += 1
    counts = np.array([len(l) for l in lists], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    members = np.array([i for l in lists for i in l], dtype=np.int64)
    return counts, offsets, members, outside


# ------------------------------------------------------------------------------------------------------------------ centroids
def centroids(f, best, counts, offsets, members, centres_old):
    """-> (centres float64 [K, E], norm [K], medoid int64 [K], written bool [K]); a centre is written when the cluster has members and
    norm >= GUARD (the guard is applied to the float64 norm here), else the old row stays."""
    f64 = np.asarray(f, dtype=np.float64)
    K = len(counts)
    centres = np.array(centres_old, dtype=np.float64, copy=True)
    norm = np.zeros(K)
    medoid = np.full(K, -1, dtype=np.int64)
    written = np.zeros(K, dtype=bool)
    for c in range(K):
        rows = members[offsets[c]:offsets[c + 1]]
        if len(rows) == 0:
            continue
        s = f64[rows].sum(0)
        norm[c] = np.sqrt((s * s).sum())
        if norm[c] >= GUARD:
            centres[c] = s / norm[c]
            written[c] = True
        bs, bi = NEG_INF, -1
        for r in rows.tolist():                                 # largest best, ties to the lowest row: `better` with the row as the index
            if better(float(best[r]), r, bs, bi):
                bs, bi = float(best[r]), r
        medoid[c] = bi
    return centres, norm, medoid, written


def centroid_cap(f, counts, offsets, members):
    """Per cluster and component, the error bound of a plain sequential fp32 sum of the members, relative to the length of the sum:
    n_c 2^-24 sum|x_i| / |sum x_i| -> float64 [K, E] (inf where the sum vanishes)."""
    f64 = np.asarray(f, dtype=np.float64)
    K = len(counts)
    cap = np.zeros((K, f64.shape[1]))
    for c in range(K):
        rows = members[offsets[c]:offsets[c + 1]]
        if len(rows) == 0:
            continue
        s = f64[rows].sum(0)
        nr = np.sqrt((s * s).sum())
        with np.errstate(divide="ignore"):
            cap[c] = len(rows) * 2.0 ** -24 * np.abs(f64[rows]).sum(0) / nr
    return cap


# ------------------------------------------------------------------------------------------------------------------ farthest first
def first_row(N, first=None, seed=0) -> int:
    return int(first) if first is not None else int(np.random.default_rng(seed).integers(N))


def farthest_first(f, n, first=None, seed=0):
    """-> (rows int64 [n], similarity float64 [n], margins float64 [n - 1]): pick j + 1 is the row least similar to its nearest earlier pick
    (NaN rows excluded, picked rows excluded, ties to the lowest row); similarity[j] = that similarity (-inf for pick 0); margins[j] =
    runner-up's value minus the pick's (inf when there is no runner-up)."""
    f64 = np.asarray(f, dtype=np.float64)
    N = f64.shape[0]
    rows = [first_row(N, first, seed)]
    sim = [NEG_INF]
    margins = []
    best = np.full(N, NEG_INF)
    idx = np.full(N, -1, dtype=np.int64)
    picked = np.zeros(N, dtype=bool)
    for j in range(n):
        picked[rows[j]] = True
        best, idx, _ = assign(f64, f64[rows[j]:rows[j] + 1], c0=j, state=(best, idx) if j else None)
        if j + 1 == n:
            break
        val = np.where(np.isnan(best), np.finfo(np.float32).max, best)
        val = np.where(picked, np.inf, val)
        nxt = int(np.argmin(val))                                # (numpy: the first of equal minima)
        others = np.delete(val, nxt)
        margins.append(float(others.min() - val[nxt]) if others.size else np.inf)
        rows.append(nxt)
        sim.append(float(best[nxt]))
    return np.array(rows, dtype=np.int64), np.array(sim), np.array(margins)


# ------------------------------------------------------------------------------------------------------------------ k-means
def reseed_rows(best, n_bad):
    """Rows for the bad clusters in order: the e-th takes the row with the e-th lowest best (NaN lowest, -0 = +0, ties to the lowest row)."""
    b = np.asarray(best, dtype=np.float64)
    key = np.where(np.isnan(b), -np.inf, b + 0.0)
    nan_first = np.where(np.isnan(b), 0, 1)
    order = np.lexsort((np.arange(len(b)), key, nan_first))      # (last key is the primary one)
    return order[:n_bad]


def kmeans(f, k, iters=20, init="farthest", seed=0):
    """Spherical k-means as spmm_amd.cluster.kmeans runs it -> dict of the Clustering's fields plus `margins` (per iteration, min over rows
    of best - second) and `init_margins` (farthest-first)."""
    f64 = np.asarray(f, dtype=np.float64)
    N = f64.shape[0]
    init_margins = np.array([])
    if init == "farthest":
        rows, _, init_margins = farthest_first(f64, k, seed=seed)
    elif init == "random":
        rows = np.random.default_rng(seed).choice(N, size=k, replace=False)
    else:
        raise ValueError(init)
    centres = f64[rows].copy()
    prev = np.full(N, -1, dtype=np.int64)
    out = dict(objective=[], margins=[], reseeded=0, init_margins=init_margins, init_rows=np.asarray(rows))
    for it in range(iters):
        best, idx, second = assign(f64, centres)
        changed = int((idx != prev).sum())
        counts, offsets, members, _ = group(idx, k)
        new, norm, medoid, written = centroids(f64, best, counts, offsets, members, centres)
        bad = np.nonzero(~written)[0]
        if len(bad):
            new[bad] = f64[reseed_rows(best, len(bad))]
            out["reseeded"] += len(bad)
        out["objective"].append(float(best.sum()))
        out["margins"].append(float((best - second).min()))
        out.update(centres=new, assign=idx, best=best, counts=counts, offsets=offsets, members=members, medoid=medoid, norm=norm,
                   iterations=it + 1, changed=changed)
        if changed == 0:
            break
        centres, prev = new, idx
    return out


# ------------------------------------------------------------------------------------------------------------------ the shared inputs
def unit_rows(n, E, seed):
    x = np.random.default_rng(seed).standard_normal((n, E))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


PLANTED_SEED = 5


def planted_mixture(seed=PLANTED_SEED, N=2000, E=64, k=8, noise=0.01):
    """k well-separated directions (orthonormal, from a QR), N rows = a direction + small noise, normalised -> (f fp32 [N, E], label [N])."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((E, E)))
    dirs = q[:, :k].T
    label = rng.integers(k, size=N)
    x = dirs[label] + noise * rng.standard_normal((N, E))
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), label


PICK_SEED = 3


def pick_rows(seed=PICK_SEED, N=500, E=64):
    return unit_rows(N, E, seed)


# ------------------------------------------------------------------------------------------------------------------ the checks
# What tests/test_cluster_kernels_gpu.py asserts of the kernels' outputs; tests/test_cluster_reference_cpu.py shows that each of them
# rejects a seeded defect.  Every function returns the deviation it measured.
def check_assign(best, idx, f, c, delta, c0=0):
    """Rows and centres without NaN: |best - float64 score of the chosen centre| <= delta, that score within delta of the float64
    maximum, and the chosen centre is the lowest-indexed of its exact copies."""
    S = scores64(f, c)
    best, idx = np.asarray(best, dtype=np.float64), np.asarray(idx, dtype=np.int64) - c0
    n, Kc = S.shape
    assert idx.shape == (n,) and bool(((idx >= 0) & (idx < Kc)).all()), "an assignment outside the chunk"
    at = S[np.arange(n), idx]
    err = float(np.abs(best - at).max()) if n else 0.0
    short = float((S.max(1) - at).max()) if n else 0.0
    assert err <= delta, ("best against float64", err, delta)
    assert short <= delta, ("the chosen centre is not the nearest", short, delta)
    c32 = np.ascontiguousarray(np.asarray(c, dtype=np.float32))
    first = {}
    for j in range(Kc):
        first.setdefault(c32[j].tobytes(), j)
    lowest = np.array([first[c32[j].tobytes()] for j in range(Kc)])
    assert bool((lowest[idx] == idx).all()), "a copy of the chosen centre has a lower index"
    return max(err, short)


def check_same_bits(a, b, what=""):
    a_best, a_idx = np.asarray(a[0], dtype=np.float32), np.asarray(a[1], dtype=np.int64)
    b_best, b_idx = np.asarray(b[0], dtype=np.float32), np.asarray(b[1], dtype=np.int64)
    assert np.array_equal(a_best.view(np.int32), b_best.view(np.int32)), f"best differs in its bits {what}"
    assert np.array_equal(a_idx, b_idx), f"assign differs {what}"


def check_group(counts, offsets, members, outside, assign_, K):
    rc, ro, rm, rout = group(assign_, K)
    assert np.array_equal(np.asarray(counts, dtype=np.int64), rc), "counts"
    assert np.array_equal(np.asarray(offsets, dtype=np.int64), ro), "offsets"
    m = np.asarray(members, dtype=np.int64)[:ro[K]]
    for c in range(K):
        seg = m[ro[c]:ro[c + 1]]
        assert bool((np.diff(seg) > 0).all()), f"members of cluster {c} do not ascend"
    assert np.array_equal(m, rm), "members"
    assert int(outside) == rout, "rows outside every cluster"


def check_centroids(centres, norm, medoid, f, best, counts, offsets, members, old, tol):
    """Centres and norms within tol of float64 (norms relative to their size) and under the sequential-sum cap; an unwritten centre
    bitwise the old one; medoids exact.  -> the largest deviation."""
    counts, offsets, members = (np.asarray(a, dtype=np.int64) for a in (counts, offsets, members))
    rc, rn, rm, written = centroids(f, best, counts, offsets, members, np.asarray(old, dtype=np.float64))
    cap = centroid_cap(f, counts, offsets, members)
    centres, old = np.asarray(centres, dtype=np.float32), np.asarray(old, dtype=np.float32)
    assert np.array_equal(np.asarray(medoid, dtype=np.int64), rm), ("medoid", np.asarray(medoid).tolist()[:8], rm.tolist()[:8])
    worst = 0.0
    for c in range(len(counts)):
        if not written[c]:
            assert np.array_equal(centres[c].view(np.int32), old[c].view(np.int32)), f"the centre of cluster {c} was written"
            continue
        err = np.abs(centres[c].astype(np.float64) - rc[c])
        # (s + ds) / |s + ds|: the component's own error, the norm's (at most |ds| / |s|), and the roundings of the squares' tree, the root
        # and the division (2^-20 covers a 512-leaf tree)
        bound = cap[c] + np.sqrt((cap[c] ** 2).sum()) + 2.0 ** -20
        assert bool((err <= bound).all()), (c, float(err.max()), float(bound.min()))
        nerr = abs(float(norm[c]) / rn[c] - 1.0)
        assert nerr <= np.sqrt((cap[c] ** 2).sum()) + 2.0 ** -20, (c, nerr)
        worst = max(worst, float(err.max()), nerr)
    for c in np.nonzero(counts == 0)[0]:
        assert float(norm[c]) == 0.0, f"norm of the empty cluster {c}"
    assert worst <= tol, ("centres / norms against float64", worst, tol)
    return worst
