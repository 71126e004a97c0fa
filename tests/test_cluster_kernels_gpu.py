"""csrc/cluster.hip against float64 (tests/kmeans_reference.py) and against spmm_sim_topk with the roles swapped.

Tiling of spmm_centroid_assign: a workgroup owns 128 rows -- four waves of two 16-row MFMA blocks -- and walks the centres in LDS tiles of
32 (two 16-centre blocks; 16 at E = 512).  So the ragged edges are n mod 16, n mod 32 (a wave), n mod 128 (a workgroup) and K mod 16,
K mod 32: n in {1, 63, 64, 65, 255, 256, 257, 1000} x K in {1, 15, 16, 17, 64, 65, 300} covers a lone row, one row short of / past a
workgroup boundary (two and three workgroups), a half-filled block, and a lone centre, a centre short of / past a block, two full tiles,
one past them, and ten tiles with a 12-centre tail.  42 of the 112 (E, n, K) triples run: every n and every K at both E.
spmm_cluster_centroids cuts a cluster into pieces of 256 members: the 5 000-member cluster is 20 pieces.

Outputs sit in sentinel-padded buffers, workspaces are NaN-filled, operands have row strides above E, every launch runs twice for bit
equality.  Tolerances: kmeans_reference.DELTA / CENTROID_TOL (four times the measured deviation, under the caps named there); every case
prints its deviation on a `[tol]` line."""
import numpy as np
import pytest
import torch

import kmeans_reference as R
from helpers_gpu import _strided

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 255, 256, 257, 1000]
KS = [1, 15, 16, 17, 64, 65, 300]
ASSIGN_CASES = [(64, n, K) for i, n in enumerate(NS) for j, K in enumerate(KS) if (i + j) % 2 == 0] + \
               [(256, n, K) for i, n in enumerate(NS) for j, K in enumerate(KS) if (i + j) % 4 == 1]
PAD = 16


def _state(n, best0=7.0, idx0=12345):
    """Sentinel-padded best / assign: the kernel writes the middle n entries only."""
    b = torch.full((n + 2 * PAD,), best0, dtype=torch.float32, device="cuda")
    a = torch.full((n + 2 * PAD,), idx0, dtype=torch.int32, device="cuda")
    return b, a


def _pads_intact(b, a, n, best0=7.0, idx0=12345):
    assert bool((b[:PAD] == best0).all()) and bool((b[PAD + n:] == best0).all()), "best written outside its rows"
    assert bool((a[:PAD] == idx0).all()) and bool((a[PAD + n:] == idx0).all()), "assign written outside its rows"


def _assign(f, c, cuts=(), c0=0, prev=None, changed=None, state=None):
    """One call, or the centre list cut at `cuts` with merge = 1 from the second piece on -> (best, assign) as numpy."""
    from spmm_amd import ops
    n = f.shape[0]
    b, a = _state(n)
    bv, av = b[PAD:PAD + n], a[PAD:PAD + n]
    if state is not None:
        bv.copy_(state[0]), av.copy_(state[1])
    edges = [0] + list(cuts) + [c.shape[0]]
    for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        last = i == len(edges) - 2
        ops.centroid_assign(f, c[lo:hi], bv, av, c0=c0 + lo, merge=(i > 0 or state is not None), prev=prev if last else None,
                            changed=changed if last else None)
    torch.cuda.synchronize()
    _pads_intact(b, a, n)
    return bv.cpu().numpy(), av.cpu().numpy()


def _topk1(f, c, base=0):
    """spmm_sim_topk(q = rows, f = centres, k = 1)."""
    from spmm_amd import ops
    n = f.shape[0]
    s = torch.full((n, 1), 7.0, dtype=torch.float32, device="cuda")
    i = torch.full((n, 1), 12345, dtype=torch.int64, device="cuda")
    ops.sim_topk(f, c, s, i, base=base, merge=False)
    torch.cuda.synchronize()
    return s[:, 0].cpu().numpy(), i[:, 0].cpu().numpy()


@pytest.mark.parametrize("E,n,K", ASSIGN_CASES, ids=[f"E{e}-n{n}-K{k}" for e, n, k in ASSIGN_CASES])
def test_assign(E, n, K):
    f32, c32 = R.unit_rows(n, E, 100 + n), R.unit_rows(K, E, 200 + K)
    if K >= 2:
        c32[K - 1] = c32[0]                               # (c) exact copies: a pair that straddles every cut below
    if K >= 17:
        c32[9] = c32[3]
    f, c = _strided(f32, 8, 4), _strided(c32, 12, 8)
    one = _assign(f, c)
    R.check_same_bits(one, _assign(f, c), "between two launches")
    R.check_same_bits(one, _topk1(f, c), "from spmm_sim_topk(k = 1)")                    # (a)
    dev = R.check_assign(one[0], one[1], f32, c32, float("inf"))
    print(f"[tol] assign E={E} n={n} K={K}: deviation {dev:.3e} delta {R.DELTA[E]:.3e} cap {R.DELTA_CAP[E]:.3e}")
    R.check_assign(one[0], one[1], f32, c32, R.DELTA[E])                                   # (b), (c)
    assert R.DELTA[E] <= R.DELTA_CAP[E]
    for cut in sorted({1, 16, 17, K - 1}):                                                 # (d)
        if 0 < cut < K:
            R.check_same_bits(one, _assign(f, c, cuts=[cut]), f"with the centres cut at {cut}")
    if K >= 65:
        R.check_same_bits(one, _assign(f, c, cuts=[1, 16, 17, K - 1]), "with the centres cut in five")
        based = _assign(f, c, cuts=[17], c0=1000)
        R.check_same_bits(based, _topk1(f, c, base=1000), "with c0 = 1000")
        assert np.array_equal(based[1], one[1] + 1000)


def test_assign_widest_feature():
    """E = 512: the instantiation with one centre block per LDS tile."""
    n, K, E = 257, 65, 512
    f32, c32 = R.unit_rows(n, E, 31), R.unit_rows(K, E, 32)
    c32[40] = c32[2]
    f, c = _strided(f32, 8, 4), _strided(c32, 12, 8)
    one = _assign(f, c)
    R.check_same_bits(one, _assign(f, c), "between two launches")
    R.check_same_bits(one, _topk1(f, c), "from spmm_sim_topk(k = 1)")
    R.check_same_bits(one, _assign(f, c, cuts=[16, 17]), "with the centres cut")
    R.check_assign(one[0], one[1], f32, c32, R.DELTA_CAP[E])


def test_assign_special_scores():
    """(e) a NaN row, an all-zero row, a -0 score, a NaN centre, and the empty / NaN states under merge = 1 -- as spmm_sim_topk orders them."""
    E, n, K = 64, 70, 20
    f32, c32 = R.unit_rows(n, E, 41), R.unit_rows(K, E, 42)
    f32[5] = np.nan                       # every score NaN: the lowest centre index, best NaN
    f32[6] = 0.0                          # every score +-0: equal scores, the lowest index, best +0
    f32[7] = 0.0
    f32[7, 0] = 1.0
    c32[:, 0] = -np.abs(c32[:, 0])        # row 7's scores are the centres' first components, all <= 0 ...
    c32[4, 0] = -0.0                      # ... and centre 4's is -0: the largest, returned as +0
    c32[11] = np.nan                      # a NaN centre never wins against a number
    f, c = _strided(f32, 8, 4), _strided(c32, 12, 8)
    best, idx = _assign(f, c)
    R.check_same_bits((best, idx), _topk1(f, c), "from spmm_sim_topk(k = 1)")
    assert np.isnan(best[5]) and idx[5] == 0
    assert best[6] == 0.0 and not np.signbit(best[6]) and idx[6] == 0
    assert best[7] == 0.0 and not np.signbit(best[7]) and idx[7] == 4
    assert not (idx[np.arange(n) != 5] == 11).any()
    keep = [i for i in range(n) if i != 5]
    ck = [j for j in range(K) if j != 11]
    S = R.scores64(f32[keep], c32[ck])
    assert np.array_equal(np.array(ck)[S.argmax(1)], idx[keep])
    # merge = 1: the empty state loses to everything, a NaN state to every number, a state that ties wins by its lower index
    st_best = torch.full((n,), float("-inf"), device="cuda")
    st_idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    st_best[1], st_idx[1] = float("nan"), 3
    st_best[2], st_idx[2] = float(best[2]), 2           # a tie with the chunk's best (index + 100 below): the state's lower index wins
    st_best[3], st_idx[3] = 2.0, 7                      # a better state stays
    st_best[5], st_idx[5] = float("nan"), 50            # NaN against NaN: the lower index (the state's)
    st_best[6], st_idx[6] = -0.0, 5                     # -0 ties with the zero row's +0: the state's lower index, returned as +0
    got = _assign(f, c, c0=100, state=(st_best, st_idx))
    exp_best, exp_idx = best.copy(), idx + 100
    exp_idx[2] = 2
    exp_best[3], exp_idx[3] = 2.0, 7
    exp_idx[5] = 50
    exp_idx[6] = 5
    R.check_same_bits(got, (exp_best, exp_idx), "after a merge with a prepared state")


def test_assign_changed_count():
    """(f) changed += rows whose assignment differs from prev: against a host count, 0 for prev = the result, summed over two calls."""
    E, n, K = 64, 1000, 65
    f32, c32 = R.unit_rows(n, E, 51), R.unit_rows(K, E, 52)
    f, c = _strided(f32, 8, 4), _strided(c32, 12, 8)
    best, idx = _assign(f, c)
    rng = np.random.default_rng(53)
    prev_h = idx.copy()
    moved = rng.choice(n, size=137, replace=False)
    prev_h[moved] = (prev_h[moved] + 1) % K
    prev = torch.from_numpy(prev_h.astype(np.int32)).cuda()
    changed = torch.zeros(1, dtype=torch.int32, device="cuda")
    R.check_same_bits((best, idx), _assign(f, c, cuts=[17], prev=prev, changed=changed), "with prev / changed given")
    assert int(changed.item()) == 137
    _assign(f, c, prev=prev, changed=changed)
    assert int(changed.item()) == 274
    same = torch.from_numpy(idx.astype(np.int32)).cuda()
    _assign(f, c, prev=same, changed=changed)
    assert int(changed.item()) == 274
    never = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _assign(f, c, prev=never, changed=changed)
    assert int(changed.item()) == 274 + n


def test_assign_no_rows():
    from spmm_amd import ops
    c = _strided(R.unit_rows(5, 64, 1), 12, 8)
    b, a = _state(0)
    ops.centroid_assign(torch.empty(0, 64, device="cuda"), c, b[PAD:PAD], a[PAD:PAD])
    torch.cuda.synchronize()
    _pads_intact(b, a, 0)


# ------------------------------------------------------------------------------------------------------------------ group
def _group(assign_h, K):
    from spmm_amd import ops
    n = len(assign_h)
    a = torch.from_numpy(np.asarray(assign_h, dtype=np.int32)).cuda()
    outs = []
    for _ in range(2):
        counts = torch.full((K + 2 * PAD,), -7, dtype=torch.int32, device="cuda")
        offsets = torch.full((K + 1 + 2 * PAD,), -7, dtype=torch.int64, device="cuda")
        members = torch.full((n + 2 * PAD,), -7, dtype=torch.int32, device="cuda")
        outside = torch.full((1 + 2 * PAD,), -7, dtype=torch.int32, device="cuda")
        ws = ops.cluster_group_workspace(n, K, "cuda")
        ws.view(torch.float32)[:] = float("nan")
        ops.cluster_group(a, K, counts[PAD:PAD + K], offsets[PAD:PAD + K + 1], members[PAD:PAD + n], outside[PAD:PAD + 1], ws=ws)
        torch.cuda.synchronize()
        for t, m in ((counts, K), (offsets, K + 1), (members, n), (outside, 1)):
            assert bool((t[:PAD] == -7).all()) and bool((t[PAD + m:] == -7).all()), "written outside the output"
        outs.append(tuple(t[PAD:PAD + m].cpu().numpy() for t, m in ((counts, K), (offsets, K + 1), (members, n), (outside, 1))))
    for x, y in zip(*outs):
        assert np.array_equal(x, y), "two launches differ"
    return outs[0]


GROUP_CASES = [(K, n, kind) for K in (1, 2, 300, 4097) for n in (0, 1, 257, 5000) for kind in ("random", "one")]


@pytest.mark.parametrize("K,n,kind", GROUP_CASES, ids=[f"K{k}-n{n}-{kind}" for k, n, kind in GROUP_CASES])
def test_group(K, n, kind):
    rng = np.random.default_rng(K * 7 + n)
    if kind == "one":
        a = np.full(n, K - 1, dtype=np.int64)                       # every row in one cluster, every other cluster empty
    else:
        a = rng.integers(-1, K + 1, size=n)                           # -1 (the empty slot) and K (past the list) are in no cluster
        a[rng.random(n) < 0.3] = K // 2                               # one heavy cluster; with K > n most clusters are empty
    counts, offsets, members, outside = _group(a, K)
    R.check_group(counts, offsets, members, outside[0], a, K)
    assert bool((members[offsets[K]:] == -7).all()), "members written past offsets[K]"


# ------------------------------------------------------------------------------------------------------------------ centroids
def _centroid_case(E):
    """Clusters of 0, 1, 63, 64, 65, 5 000 members, a cancelling pair, and a cluster whose members tie in best (rows in shuffled order)."""
    sizes = [0, 1, 63, 64, 65, 5000, 2, 40, 0]
    rng = np.random.default_rng(61 + E)
    a = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)] + [np.full(9, -1)])
    rng.shuffle(a)
    n = len(a)
    f32 = R.unit_rows(n, E, 62 + E)
    dirs = R.unit_rows(len(sizes), E, 63 + E)
    f32 = f32 * 0.3 + dirs[np.clip(a, 0, None)]                        # members lean towards their cluster's direction
    f32 = (f32 / np.linalg.norm(f32, axis=1, keepdims=True)).astype(np.float32)
    pair = np.nonzero(a == 6)[0]
    f32[pair[1]] = -f32[pair[0]]                                       # v, -v: the sum is exactly zero
    best = rng.random(n).astype(np.float32)
    tied = np.nonzero(a == 7)[0]
    best[tied] = 0.25
    best[tied[[5, 17, 30]]] = 0.75                                      # three members share the largest best: the lowest row
    big = np.nonzero(a == 5)[0]
    best[big[[10, 4000]]] = 2.0                                         # a tie across two pieces of the large cluster
    best[np.nonzero(a == 3)[0][0]] = np.nan                             # NaN is the lowest best
    return a, f32, best, len(sizes)


@pytest.mark.parametrize("E", [64, 256, 100])
def test_centroids(E):
    from spmm_amd import ops
    a, f32, best, K = _centroid_case(E)
    n = len(a)
    counts_h, offsets_h, members_h, _ = R.group(a, K)
    f = _strided(f32, 8, 4)
    old32 = R.unit_rows(K, E, 64)
    counts = torch.from_numpy(counts_h.astype(np.int32)).cuda()
    offsets = torch.from_numpy(offsets_h).cuda()
    members = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    members[:len(members_h)] = torch.from_numpy(members_h.astype(np.int32)).cuda()
    best_d = torch.from_numpy(best).cuda()
    outs = []
    for _ in range(2):
        wide = torch.full((K + 2, E + 12), 9.0, device="cuda")
        centres = wide[1:K + 1, 8:8 + E]
        centres.copy_(torch.from_numpy(old32))
        norm = torch.full((K + 2 * PAD,), -7.0, device="cuda")
        medoid = torch.full((K + 2 * PAD,), -7, dtype=torch.int32, device="cuda")
        ws = ops.cluster_centroids_workspace(n, K, E, "cuda")
        ws.view(torch.float32)[:] = float("nan")
        ops.cluster_centroids(f, best_d, counts, offsets, members, centres, norm[PAD:PAD + K], medoid[PAD:PAD + K], ws=ws)
        torch.cuda.synchronize()
        assert bool((wide[0] == 9.0).all()) and bool((wide[K + 1] == 9.0).all()) and bool((wide[:, :8] == 9.0).all()) \
            and bool((wide[:, 8 + E:] == 9.0).all()), "centres written outside their rows"
        assert bool((norm[:PAD] == -7).all()) and bool((norm[PAD + K:] == -7).all()) and bool((medoid[:PAD] == -7).all()) \
            and bool((medoid[PAD + K:] == -7).all())
        outs.append((centres.cpu().numpy().copy(), norm[PAD:PAD + K].cpu().numpy(), medoid[PAD:PAD + K].cpu().numpy()))
    for x, y in zip(*outs):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), "two launches differ"
    cen, nrm, med = outs[0]
    dev = R.check_centroids(cen, nrm, med, f32, best, counts_h, offsets_h, members_h, old32, float("inf"))
    print(f"[tol] centroids E={E}: deviation {dev:.3e} tolerance {R.CENTROID_TOL:.3e}")
    R.check_centroids(cen, nrm, med, f32, best, counts_h, offsets_h, members_h, old32, R.CENTROID_TOL)
    assert med[0] == -1 and med[8] == -1 and nrm[6] == 0.0
