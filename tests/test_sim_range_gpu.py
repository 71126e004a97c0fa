"""spmm_sim_range (csrc/neighbors.hip) against brute-force float64 lists (tests/butina_reference.py) and, bit for bit, against
spmm_sim_topk's scores.

Tiling: a workgroup owns 128 rows -- four waves of two 16-row MFMA blocks -- and walks the columns in LDS tiles of 32 (two 16-column
blocks; 16 at E = 512); a row's hits of a tile sit in four lanes.  So the edges are n mod 16 / 32 / 128 and nc mod 16 / 32.

Operands sit inside wider NaN-filled matrices (row stride above E, offset start), counts and nbr in sentinel-padded buffers, every launch
sequence runs twice for bit equality.  With a picked threshold (butina_reference.pick_threshold) every pair is decided alike in fp32 and
float64, so the lists are compared exactly; the deviation of the scores themselves is printed on a `[tol]` line by the boundary test."""
import numpy as np
import pytest
import torch

import butina_reference as B
from helpers_gpu import _strided

pytestmark = pytest.mark.gpu

PAD = 16
C_PAD, N_PAD = 12345, -777


def _sweep(f, c, t, r0, c0, col_cuts, row_cuts, offsets, nbr_len):
    """Every (row piece, column piece) in ascending order into fresh sentinel-padded buffers -> (counts [n], nbr buffer or None)."""
    from spmm_amd import ops
    n, nc = f.shape[0], c.shape[0]
    cb = torch.full((n + 2 * PAD,), C_PAD, dtype=torch.int32, device="cuda")
    cv = cb[PAD:PAD + n]
    cv.zero_()
    nb = nv = None
    if offsets is not None:
        total = int(offsets[-1])
        nb = torch.full((total + 2 * PAD,), N_PAD, dtype=torch.int32, device="cuda")
        nv = nb[PAD:PAD + nbr_len]
    redges, cedges = [0] + list(row_cuts) + [n], [0] + list(col_cuts) + [nc]
    for rlo, rhi in zip(redges[:-1], redges[1:]):
        for clo, chi in zip(cedges[:-1], cedges[1:]):
            ops.sim_range(f[rlo:rhi], c[clo:chi], t, cv[rlo:rhi], r0=r0 + rlo, c0=c0 + clo,
                          offsets=None if offsets is None else offsets[rlo:rhi], nbr=nv)
    torch.cuda.synchronize()
    assert bool((cb[:PAD] == C_PAD).all()) and bool((cb[PAD + n:] == C_PAD).all()), "counts written outside its rows"
    return cv.cpu().numpy(), nb


def _lists(f, c, t, r0=0, c0=0, col_cuts=(), row_cuts=(), short=0):
    """The count pass, the cumsum, the emit pass -- each twice -> (counts, offsets, nbr [M - short]) as numpy."""
    counts, _ = _sweep(f, c, t, r0, c0, col_cuts, row_cuts, None, 0)
    again, _ = _sweep(f, c, t, r0, c0, col_cuts, row_cuts, None, 0)
    assert np.array_equal(counts, again), "two count passes differ"
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    M = int(offsets[-1])
    off = torch.from_numpy(offsets).cuda()
    keep = max(M - short, 0)
    got = []
    for _ in range(2):
        emitted, nb = _sweep(f, c, t, r0, c0, col_cuts, row_cuts, off, keep)
        assert np.array_equal(emitted, counts), "the emit pass's counts are not the count pass's"
        nb = nb.cpu().numpy()
        assert (nb[:PAD] == N_PAD).all() and (nb[PAD + keep:] == N_PAD).all(), "nbr written outside [0, nbr_len)"
        got.append(nb[PAD:PAD + keep])
    assert got[0].tobytes() == got[1].tobytes(), "two emit passes differ"
    return counts, offsets, got[0]


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"counts differ {what}"
    assert a[2].tobytes() == b[2].tobytes(), f"nbr differs {what}"


COMPLETE = [(64, n) for n in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)] + [(256, 65), (256, 257), (512, 129)]


@pytest.mark.parametrize("E,n", COMPLETE, ids=[f"E{e}-n{n}" for e, n in COMPLETE])
def test_complete_and_empty_relations_are_exact(E, n):
    """threshold -2: every row's list is all j != i, ascending -- the diagonal exclusion and the order at every tile position; threshold 2:
    nothing is written."""
    x = B.R.unit_rows(n, E, seed=n + E)
    f = _strided(x, 8, 4)
    counts, offsets, nbr = _lists(f, f, -2.0)
    B.check_lists(counts, offsets, nbr, B.complete(n), "at threshold -2")
    counts, offsets, nbr = _lists(f, f, 2.0)
    assert not counts.any() and nbr.size == 0


def _topk_scores(f):
    """All n <= 64 scores of every row from spmm_sim_topk(k = n) as a matrix of fp32 values."""
    from spmm_amd import ops
    n = f.shape[0]
    s = torch.empty((n, n), dtype=torch.float32, device="cuda")
    i = torch.empty((n, n), dtype=torch.int64, device="cuda")
    ops.sim_topk(f, f, s, i, base=0, merge=False)
    torch.cuda.synchronize()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    out = np.empty((n, n), dtype=np.float32)
    for r in range(n):
        assert sorted(i[r].tolist()) == list(range(n))
        out[r, i[r]] = s[r]
    return out


@pytest.mark.parametrize("E", [64, 256])
def test_inclusive_boundary_is_bit_exact_against_sim_topk(E):
    """The threshold is the fp32 score of one pair: the lists are exactly {j != i : score bits >= threshold}, hold that pair in both
    directions and are symmetric."""
    n = 64
    x = B.R.unit_rows(n, E, seed=7 + E)
    f = _strided(x, 8, 4)
    G = _topk_scores(f)
    assert np.array_equal(G.view(np.int32), G.T.copy().view(np.int32)), "spmm_sim_topk's scores are not symmetric in their bits"
    err = np.abs(G.astype(np.float64) - B.cosines64(x))
    dev = float(err[~np.eye(n, dtype=bool)].max())                              # (the pairs a list can hold; the diagonal is printed only)
    print(f"[tol] sim_range E={E} n={n}: deviation of the scores its lists are bit-exact to {dev:.3e} (diagonal {float(err.max()):.3e}) "
          f"delta {B.DELTA[E]:.3e} cap {B.DELTA_CAP[E]:.3e}")
    assert dev <= B.DELTA[E] <= B.DELTA_CAP[E]
    off = G[~np.eye(n, dtype=bool)]
    want_level = np.sort(off)[int(0.9 * off.size)]
    i0, j0 = np.argwhere((G == want_level) & ~np.eye(n, dtype=bool))[0]
    t = float(G[i0, j0])
    want = [[j for j in range(n) if j != i and G[i, j] >= np.float32(t)] for i in range(n)]
    assert j0 in want[i0] and i0 in want[j0] and B.symmetric(want) and 0 < sum(map(len, want)) < n * (n - 1)
    counts, offsets, nbr = _lists(f, f, t)
    B.check_lists(counts, offsets, nbr, want, "against spmm_sim_topk's bits")
    above = np.nextafter(np.float32(t), np.float32(2))
    strict = [[j for j in range(n) if j != i and G[i, j] >= above] for i in range(n)]
    assert strict != want
    B.check_lists(*_lists(f, f, float(above)), strict, "one ulp above the pair's score")


@pytest.mark.parametrize("n,E", B.RANGE_CASES, ids=[f"n{n}-E{e}" for n, e in B.RANGE_CASES])
def test_lists_against_float64_with_a_picked_threshold(n, E):
    """Random unit rows with exact copies (rows 0, 3, n - 1), a NaN row and a zero row: sets equal, lists ascending, emit counts = counts."""
    x, S, t, margin = B.range_input(n, E)
    assert margin >= B.DELTA[E] and B.DELTA[E] <= B.DELTA_CAP[E]
    want = B.neighbour_lists(S, t)
    f = _strided(x, 8, 4)
    counts, offsets, nbr = _lists(f, f, t)
    B.check_lists(counts, offsets, nbr, want, f"at the picked threshold {t!r}")
    got = B.uncsr(counts, offsets, nbr)
    assert got[5] == [] and all(5 not in l for l in got), "the NaN row has no neighbours and is nobody's"
    assert {3, n - 1} <= set(got[0]) and B.symmetric(got)


def test_any_chunking_gives_the_same_bytes():
    n, E = 257, 64
    x, S, t, _ = B.range_input(n, E)
    f = _strided(x, 8, 4)
    c = _strided(x, 12, 8)
    one = _lists(f, c, t)
    B.check_lists(*one, B.neighbour_lists(S, t))
    for cut in (1, 16, 17, n - 1):
        _same(one, _lists(f, c, t, col_cuts=[cut]), f"with the columns cut at {cut}")
    _same(one, _lists(f, c, t, col_cuts=[1, 16, 17, n - 1]), "with the columns cut in five")
    for cut in (1, 127, 128, 129):
        _same(one, _lists(f, c, t, row_cuts=[cut]), f"with the rows cut at {cut}")
    _same(one, _lists(f, c, t, row_cuts=[128], col_cuts=[17, 200]), "with rows and columns cut")


def test_rectangular_calls_exclude_only_equal_library_indices():
    n, E = 257, 64
    x, S, t, _ = B.range_input(n, E)
    f = _strided(x[:100], 8, 4)
    c = _strided(x, 12, 8)
    for thr in (t, -2.0):
        got = _lists(f, c, thr, r0=1000, c0=0)                                  # disjoint index ranges: nothing is the diagonal
        want = B.neighbour_lists(S[:100], thr, r0=1000, c0=0)
        assert all(i in want[i] for i in range(100) if i not in (5, 7)), "a row's own copy on the column side is a neighbour"
        B.check_lists(*got, want, "with disjoint ranges")
        got = _lists(f, c, thr, r0=50, c0=0, col_cuts=[60])                     # overlapping: exactly r0 + i == c0 + j is left out
        want = B.neighbour_lists(S[:100], thr, r0=50, c0=0)
        assert all(50 + i not in want[i] for i in range(100))
        B.check_lists(*got, want, "with overlapping ranges")
        got = _lists(f, c[20:], thr, r0=0, c0=20)
        B.check_lists(*got, B.neighbour_lists(S[:100, 20:], thr, r0=0, c0=20), "with c0 = 20")


def test_guarded_emission():
    """nbr_len 5 short of M: nothing at or past nbr_len is written, everything before it is right, the counts are complete."""
    n, E = 256, 64
    x, S, t, _ = B.range_input(n, E)
    f = _strided(x, 8, 4)
    counts, offsets, nbr = _lists(f, f, t)
    short = _lists(f, f, t, short=5)
    assert np.array_equal(short[0], counts) and short[2].size == nbr.size - 5
    assert short[2].tobytes() == nbr[:-5].tobytes()


def test_no_rows_and_no_columns_are_no_ops():
    from spmm_amd import ops
    x = B.R.unit_rows(20, 64, seed=1)
    f = _strided(x, 8, 4)
    counts = torch.full((20,), 3, dtype=torch.int32, device="cuda")
    ops.sim_range(f, f[:0], -2.0, counts)
    ops.sim_range(f[:0], f, -2.0, counts[:0])
    torch.cuda.synchronize()
    assert bool((counts == 3).all())
    ops.sim_range(f, f, -2.0, counts)
    torch.cuda.synchronize()
    assert bool((counts == 3 + 19).all()), "counts += the hits"
