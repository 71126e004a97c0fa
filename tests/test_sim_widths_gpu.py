"""Every feature width the E / 64 dispatch of csrc/sim_scan.h builds and no other test launches: E = 128, 192, 320, 384, 448 through
spmm_centroid_assign and spmm_sim_range (64, 256 and 512 run in tests/test_cluster_kernels_gpu.py and tests/test_sim_range_gpu.py, whose
helpers these cases use).

Shapes.  n = 129 rows: two workgroups, the second with one row in a half-empty block.  K = 33 centres: at these widths an LDS tile holds
two 16-centre blocks, so one full tile and a one-centre tail; centre 32 is an exact copy of centre 0 across the tile cut.  The range scan
walks the same 129 rows as columns: four full tiles and a one-column tail.

Tolerance.  No deviation has been measured at these widths, so the float64 check uses the derived cap kmeans_reference.DELTA_CAP[E] =
E 2^-23 (twice the first-order bound of an E-term fmaf chain on unit vectors), as test_assign_widest_feature does at 512: it guards
against a wrong operand.  The sharp assertions are the bit identities.  profiles/cluster_tol.txt holds the `[tol]` lines."""
import numpy as np
import pytest

import butina_reference as B
import kmeans_reference as R
from helpers_gpu import _strided
from test_cluster_kernels_gpu import _assign, _topk1
from test_sim_range_gpu import _lists, _topk_scores

pytestmark = pytest.mark.gpu

WIDTHS = [128, 192, 320, 384, 448]


@pytest.mark.parametrize("E", WIDTHS)
def test_assign_width(E):
    n, K = 129, 33
    f32, c32 = R.unit_rows(n, E, 300 + E), R.unit_rows(K, E, 400 + E)
    c32[32] = c32[0]
    f, c = _strided(f32, 8, 4), _strided(c32, 12, 8)
    one = _assign(f, c)
    R.check_same_bits(one, _assign(f, c), "between two launches")
    R.check_same_bits(one, _topk1(f, c), "from spmm_sim_topk(k = 1)")
    R.check_same_bits(one, _assign(f, c, cuts=[17]), "with the centres cut at 17")
    dev = R.check_assign(one[0], one[1], f32, c32, float("inf"))
    print(f"[tol] assign E={E} n={n} K={K}: deviation {dev:.3e} cap {R.DELTA_CAP[E]:.3e}")
    R.check_assign(one[0], one[1], f32, c32, R.DELTA_CAP[E])


@pytest.mark.parametrize("E", WIDTHS)
def test_range_width_complete_and_empty(E):
    """threshold -2: every list is all j != i, ascending, from the count pass and the emit pass; threshold 2: nothing is written."""
    n = 129
    f = _strided(B.R.unit_rows(n, E, seed=n + E), 8, 4)
    B.check_lists(*_lists(f, f, -2.0), B.complete(n), "at threshold -2")
    counts, offsets, nbr = _lists(f, f, 2.0)
    assert not counts.any() and nbr.size == 0


@pytest.mark.parametrize("E", WIDTHS)
def test_range_width_inclusive_boundary(E):
    """The threshold is one pair's fp32 score from spmm_sim_topk(k = n): the lists are exactly the pairs whose score bits are >= it, and
    one ulp above drops that pair."""
    n = 64
    x = B.R.unit_rows(n, E, seed=7 + E)
    f = _strided(x, 8, 4)
    G = _topk_scores(f)
    off_diag = ~np.eye(n, dtype=bool)
    assert np.array_equal(G.view(np.int32), G.T.copy().view(np.int32)), "spmm_sim_topk's scores are not symmetric in their bits"
    dev = float(np.abs(G.astype(np.float64) - B.cosines64(x))[off_diag].max())
    print(f"[tol] sim_range E={E} n={n}: deviation of the scores its lists are bit-exact to {dev:.3e} cap {B.DELTA_CAP[E]:.3e}")
    assert dev <= B.DELTA_CAP[E]
    level = np.sort(G[off_diag])[int(0.9 * n * (n - 1))]
    i0, j0 = np.argwhere((G == level) & off_diag)[0]
    t = np.float32(G[i0, j0])
    want = [[j for j in range(n) if j != i and G[i, j] >= t] for i in range(n)]
    assert j0 in want[i0] and i0 in want[j0] and B.symmetric(want) and 0 < sum(map(len, want)) < n * (n - 1)
    B.check_lists(*_lists(f, f, float(t)), want, "against spmm_sim_topk's bits")
    above = np.nextafter(t, np.float32(2))
    strict = [[j for j in range(n) if j != i and G[i, j] >= above] for i in range(n)]
    assert strict != want
    B.check_lists(*_lists(f, f, float(above)), strict, "one ulp above the pair's score")
