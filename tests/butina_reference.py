"""TEST INFRASTRUCTURE (never imported by spmm_amd/): threshold clustering restated in plain Python / float64 numpy -- the neighbour list
of every row by brute force, the sequential leader algorithm (Taylor-Butina and first-come), a model of the parallel rounds and of the
finish rule as csrc/neighbors.hip specifies them, the threshold picker, the inputs the GPU tests use, and the checks those tests apply
(tests/test_butina_reference_cpu.py shows that each check rejects a seeded defect).

A neighbour list is a Python list of ascending int lists here; `csr` / `uncsr` convert to and from (counts, offsets, nbr).

The bound.  A GPU score is spmm_sim_topk's accumulator chain; its deviation from float64 on unit rows is kmeans_reference.DELTA[E].  The
picker returns a threshold that every float64 pair cosine misses by at least DELTA[E], so every pair is decided the same way in fp32 and
in float64 and the neighbour sets are compared exactly, with no excluded pairs."""
from __future__ import annotations

import numpy as np

import kmeans_reference as R

DELTA, DELTA_CAP = R.DELTA, R.DELTA_CAP


# ------------------------------------------------------------------------------------------------------------------ neighbour lists
def cosines64(f, c=None):
    """float64 scores [n, nc], every entry the same sum whatever the shapes are (kmeans_reference.scores64): exactly symmetric for c = f."""
    return R.scores64(f, f if c is None else c)


def neighbour_lists(S, t, r0=0, c0=0):
    """Row i's list: c0 + j for every j with S[i, j] >= t (NaN never) and r0 + i != c0 + j, ascending."""
    t = float(t)
    out = []
    with np.errstate(invalid="ignore"):
        for i in range(S.shape[0]):
            j = np.nonzero(S[i] >= t)[0] + c0
            out.append(j[j != r0 + i].tolist())
    return out


def csr(lists):
    counts = np.array([len(l) for l in lists], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    nbr = np.array([j for l in lists for j in l], dtype=np.int32)
    return counts, offsets, nbr


def uncsr(counts, offsets, nbr):
    counts, offsets, nbr = np.asarray(counts), np.asarray(offsets), np.asarray(nbr)
    return [nbr[offsets[i]:offsets[i] + counts[i]].tolist() for i in range(len(counts))]


def symmetric(lists) -> bool:
    sets = [set(l) for l in lists]
    return all(i in sets[j] for i, l in enumerate(lists) for j in l)


# ------------------------------------------------------------------------------------------------------------------ the threshold picker
def pair_values(S):
    """The finite off-diagonal entries of a square score matrix (each pair once) or every finite entry of a rectangular one."""
    v = S[np.triu_indices(S.shape[0], 1)] if S.shape[0] == S.shape[1] else S.ravel()
    return v[np.isfinite(v)]


def pick_threshold(values, target, delta):
    """-> (threshold as an fp32 number, margin): the midpoint, rounded to fp32, of the gap of width >= 4 delta between consecutive pair
    cosines that lies nearest `target`; asserts that after the rounding every pair is still >= delta away."""
    v = np.unique(np.asarray(values, dtype=np.float64))
    assert v.size >= 2, "no two distinct pair cosines"
    gaps = np.diff(v)
    wide = np.nonzero(gaps >= 4 * delta)[0]
    assert wide.size, "no gap of 4 delta between the pair cosines"
    mid = (v[wide] + v[wide + 1]) / 2
    t = np.float32(mid[np.argmin(np.abs(mid - target))])
    margin = float(np.abs(v - float(t)).min())
    assert margin >= delta, ("a pair cosine within delta of the threshold", margin, delta)
    return float(t), margin


# ------------------------------------------------------------------------------------------------------------------ leaders
def priority_order(counts, by_count):
    n = len(counts)
    return sorted(range(n), key=(lambda i: (-int(counts[i]), i)) if by_count else (lambda i: i))


def sequential(lists, by_count, tie_high=False):
    """Visit the rows in priority order; a row not yet claimed becomes a leader and claims its unclaimed neighbours -> leader int64 [n].
    by_count: more neighbours first, equal counts to the lower row (tie_high: to the higher row -- RDKit's order, a seeded defect here)."""
    n = len(lists)
    counts = [len(l) for l in lists]
    order = priority_order(counts, by_count)
    if tie_high:
        order = sorted(range(n), key=lambda i: (-counts[i] if by_count else 0, -i))
    leader = np.full(n, -1, dtype=np.int64)
    for i in order:
        if leader[i] >= 0:
            continue
        leader[i] = i
        for j in lists[i]:
            if leader[j] < 0:
                leader[j] = i
    return leader


def _rank(lists, by_count):
    rank = np.empty(len(lists), dtype=np.int64)
    rank[priority_order([len(l) for l in lists], by_count)] = np.arange(len(lists))
    return rank


def one_round(lists, by_count, state, in_place=False):
    """state int [n] (0 open, 1 leader, 2 member) -> (the next state, rows still open).  An open row with a leader among its neighbours of
    higher priority becomes a member; one whose neighbours of higher priority are all members (or that has none) a leader; else it stays.
    in_place: the round reads its own output (a seeded defect)."""
    rank = _rank(lists, by_count)
    state = np.asarray(state, dtype=np.int64)
    new = state.copy()
    src = new if in_place else state
    for i in range(len(lists)):
        if state[i] != 0:
            continue
        higher = [j for j in lists[i] if rank[j] < rank[i]]
        if any(src[j] == 1 for j in higher):
            new[i] = 2
        elif all(src[j] == 2 for j in higher):
            new[i] = 1
    return new, int((new == 0).sum())


def rounds(lists, by_count, cap=None):
    """Rounds from the all-open state until none is open -> (state, number of rounds, [open after every round])."""
    state = np.zeros(len(lists), dtype=np.int64)
    opens = []
    while True:
        state, left = one_round(lists, by_count, state)
        opens.append(left)
        if left == 0:
            return state, len(opens), opens
        assert cap is None or len(opens) < cap, "the rounds do not end"


def finish(lists, by_count, state, lowest=False):
    """leader[i] = i for a leader, else the highest-priority leader among i's neighbours, -1 if none (lowest: the LOWEST-priority one, a
    seeded defect)."""
    rank = _rank(lists, by_count)
    out = np.full(len(lists), -1, dtype=np.int64)
    for i, l in enumerate(lists):
        if state[i] == 1:
            out[i] = i
            continue
        led = sorted((j for j in l if state[j] == 1), key=lambda j: rank[j])
        if led:
            out[i] = led[-1] if lowest else led[0]
    return out


def numbering(leader, counts, by_count):
    """-> (leaders in cluster order, cluster of every row): clusters numbered in the priority order of their leaders."""
    leader = np.asarray(leader, dtype=np.int64)
    rows = [i for i in priority_order(counts, by_count) if leader[i] == i]
    number = {r: k for k, r in enumerate(rows)}
    return np.array(rows, dtype=np.int64), np.array([number.get(int(l), -1) for l in leader], dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------ the checks
def check_lists(counts, offsets, nbr, want, what=""):
    """The kernel's (counts, offsets, nbr) against the brute-force lists: equal sets AND ascending order, so equal sequences."""
    got = uncsr(counts, offsets, nbr)
    assert len(got) == len(want), f"rows {what}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert all(a < b for a, b in zip(g, g[1:])), f"row {i}: the list does not ascend {what}: {g[:12]}"
        assert g == list(w), f"row {i}: neighbours {g[:12]} != {list(w)[:12]} {what}"


def check_round(state_out, open_out, lists, by_count, state_in, what=""):
    want, left = one_round(lists, by_count, state_in)
    assert np.array_equal(np.asarray(state_out, dtype=np.int64), want), f"state after the round {what}"
    assert int(open_out) == left, f"open rows {int(open_out)} != {left} {what}"


def check_leaders(leader, lists, by_count, what=""):
    want = sequential(lists, by_count)
    got = np.asarray(leader, dtype=np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"leader of row {bad[:5].tolist()}: {got[bad[:5]].tolist()} != {want[bad[:5]].tolist()} {what}"


# ------------------------------------------------------------------------------------------------------------------ graphs
def random_graph(n, density, seed, equal_counts=True):
    """A symmetric random graph as lists; equal_counts plants rows of equal degree (pairs of rows with each other's neighbourhoods)."""
    rng = np.random.default_rng(seed)
    a = np.triu(rng.random((n, n)) < density, 1)
    if equal_counts and n >= 4:
        for k in range(0, n - 1, max(2, n // 6)):                # row k + 1 gets row k's row above the diagonal where it can
            a[k + 1, k + 2:] = a[k, k + 2:]
    a = a | a.T
    return [np.nonzero(a[i])[0].tolist() for i in range(n)]


def path(n):
    return [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]


def star(leaves):
    return [list(range(1, leaves + 1))] + [[0] for _ in range(leaves)]


def complete(n):
    return [[j for j in range(n) if j != i] for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------ the shared inputs
RANGE_TARGET = {64: 0.2, 256: 0.12}
RANGE_CASES = [(n, E) for E in (64, 256) for n in (255, 256, 257, 1000)]
_cache = {}


def range_input(n, E):
    """Random unit rows with exact copies (rows 0, 3 and n - 1 equal), one NaN row (5) and one zero row (7) -> (f fp32 [n, E], S float64,
    threshold, margin): the threshold picked near RANGE_TARGET[E]."""
    key = ("range", n, E)
    if key not in _cache:
        f = R.unit_rows(n, E, seed=100 + n + E)
        f[3] = f[0]
        f[n - 1] = f[0]
        f[5] = np.nan
        f[7] = 0.0
        S = cosines64(f)
        t, margin = pick_threshold(pair_values(S), RANGE_TARGET[E], DELTA[E])
        _cache[key] = (f, S, t, margin)
    return _cache[key]


GROUP_SIZES = [120, 5, 64, 33, 17, 90, 8, 47, 12, 71, 47, 55]        # (two of equal size: numbered by leader row)
MIX_THRESHOLD = 0.6


def planted_groups(E=64, seed=11, noise=0.02):
    """12 groups of 5 .. 120 rows around orthonormal directions, shuffled -> (f fp32 [N, E], label [N]).  Within a group the cosine is
    above 0.9, between groups below 0.3 (asserted by the CPU test), so at threshold 0.6 a neighbourhood is the row's group."""
    key = ("groups", E, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        q, _ = np.linalg.qr(rng.standard_normal((E, E)))
        label = rng.permutation(np.repeat(np.arange(len(GROUP_SIZES)), GROUP_SIZES))
        x = q[:, :len(GROUP_SIZES)].T[label] + noise * rng.standard_normal((label.size, E))
        _cache[key] = ((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), label)
    return _cache[key]


DEDUP_THRESHOLD = 0.95


def dedup_library(E=64, seed=21, n=300):
    """Random unit rows with planted duplicate sets -> (f, first [n]): first[i] = the row i is a copy of (itself when it is an original).
    Exact copies and near copies (a perturbation of 0.05 relative length: cosine about 0.9988, above the threshold by far more than 100
    DELTA); distinct originals have |cosine| < 0.7 (asserted by the CPU test)."""
    key = ("dedup", E, seed, n)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        f = R.unit_rows(n, E, seed).astype(np.float64)
        first = np.arange(n)
        for k, src in enumerate(rng.choice(n // 2, size=20, replace=False).tolist()):
            for dst in rng.choice(np.arange(n // 2, n), size=1 + k % 3, replace=False).tolist():
                if first[dst] != dst:
                    continue
                y = f[src] if k % 2 == 0 else f[src] + 0.05 * rng.standard_normal(E) / np.sqrt(E)
                f[dst] = y / np.linalg.norm(y)
                first[dst] = src
        _cache[key] = (f.astype(np.float32), first)
    return _cache[key]
