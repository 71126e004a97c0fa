"""tests/kmeans_reference.py against brute force on tiny cases; the INPUT CONDITIONS the GPU tests rely on (every decision the reference
makes on their inputs has a float64 margin above 100 delta, so an fp32 kernel within delta of float64 must make the same decisions); and
the checks the GPU tests use, each shown to reject a seeded defect."""
import numpy as np
import pytest

import kmeans_reference as R


# ------------------------------------------------------------------------------------------------------------------ brute force
def test_assign_is_the_argmax_with_ties_to_the_lowest_index():
    f, c = R.unit_rows(40, 64, 1), R.unit_rows(9, 64, 2)
    c[7] = c[2]
    f[3] = c[2]
    best, idx, second = R.assign(f, c)
    S = R.scores64(f, c)
    assert np.array_equal(idx, S.argmax(1)) and np.array_equal(best, S.max(1)) and idx[3] == 2
    assert second[3] == best[3]                                  # the copy is the runner-up: margin 0
    b2, i2, _ = R.assign(f, c, c0=50)
    assert np.array_equal(i2, idx + 50) and np.array_equal(b2, best)


def test_assign_chunks_merge_to_one_call():
    f, c = R.unit_rows(30, 64, 3), R.unit_rows(11, 64, 4)
    c[10] = c[0]
    one = R.assign(f, c)
    for cut in (1, 5, 10):
        st = R.assign(f, c[:cut])
        got = R.assign(f, c[cut:], c0=cut, state=st[:2])
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1])


def test_order_of_special_scores():
    assert R.better(0.5, 3, 0.5, 4) and not R.better(0.5, 4, 0.5, 3)
    assert R.better(-0.0, 1, 0.0, 2) and not R.better(0.0, 2, -0.0, 1)            # -0 = +0: the index decides
    assert R.better(float("-inf"), 5, float("nan"), 1) and not R.better(float("nan"), 1, -1e30, 5)
    assert R.better(float("nan"), 1, float("nan"), 2) and R.better(float("nan"), 9, float("-inf"), -1)
    assert not R.better(1.0, -1, float("nan"), 3)
    f = np.zeros((2, 64), dtype=np.float32)
    f[1] = np.nan
    best, idx, _ = R.assign(f, R.unit_rows(3, 64, 5))
    assert best[0] == 0.0 and not np.signbit(best[0]) and idx[0] == 0 and np.isnan(best[1]) and idx[1] == 0
    empty = R.assign(f[:0], R.unit_rows(3, 64, 5))
    assert empty[0].shape == (0,)


def test_group_and_centroids_brute_force():
    rng = np.random.default_rng(6)
    a = rng.integers(-1, 6, size=200)                            # clusters 0..4 of K = 5; -1 and 5 are outside
    counts, offsets, members, outside = R.group(a, 5)
    assert outside == int(((a < 0) | (a >= 5)).sum()) and offsets[-1] == len(members) == 200 - outside
    for c in range(5):
        assert np.array_equal(members[offsets[c]:offsets[c + 1]], np.nonzero(a == c)[0]) and counts[c] == (a == c).sum()
    f = R.unit_rows(200, 64, 7)
    best = rng.random(200)
    old = R.unit_rows(5, 64, 8).astype(np.float64)
    cen, norm, med, written = R.centroids(f, best, counts, offsets, members, old)
    for c in range(5):
        rows = np.nonzero(a == c)[0]
        s = f[rows].astype(np.float64).sum(0)
        assert np.allclose(cen[c], s / np.linalg.norm(s), atol=1e-15) and abs(norm[c] - np.linalg.norm(s)) < 1e-12 and written[c]
        assert med[c] == rows[np.argmax(best[rows])]
    # an empty cluster and a cancelling pair keep the old centre
    a2 = np.array([0, 0, 2, 2, 2])
    f2 = R.unit_rows(5, 64, 9)
    f2[1] = -f2[0]
    g2 = R.group(a2, 3)
    cen2, norm2, med2, wr2 = R.centroids(f2, np.array([.1, .9, .5, .5, .2]), *g2[:3], old[:3])
    assert wr2.tolist() == [False, False, True] and np.array_equal(cen2[:2], old[:2]) and norm2[0] == 0.0
    assert med2.tolist() == [1, -1, 2]                            # ties in best: the lowest row


def test_farthest_first_brute_force():
    f = R.unit_rows(60, 64, 10)
    rows, sim, margins = R.farthest_first(f, 12, first=17)
    S = R.scores64(f, f)
    assert rows[0] == 17 and sim[0] == -np.inf and len(set(rows.tolist())) == 12
    for j in range(1, 12):
        nearest = S[:, rows[:j]].max(1)
        nearest[rows[:j]] = np.inf
        assert rows[j] == nearest.argmin() and sim[j] == nearest[rows[j]]
    assert bool((margins >= 0).all())
    assert R.farthest_first(f, 3, seed=4)[0][0] == R.first_row(60, None, 4) and R.first_row(60, 5, 4) == 5
    # duplicate rows: a copy is never picked while another row remains
    g = np.concatenate([f[:5], f[:5], f[:5]])
    rows = R.farthest_first(g, 5, first=0)[0]
    assert sorted((rows % 5).tolist()) == [0, 1, 2, 3, 4]
    # a NaN row is never picked while a number remains
    h = f[:6].copy()
    h[2] = np.nan
    assert 2 not in R.farthest_first(h, 5, first=0)[0].tolist()


def test_kmeans_reseeds_in_order_of_lowest_best():
    best = np.array([0.5, np.nan, 0.1, 0.1, -0.0, 0.0, 0.9])
    assert R.reseed_rows(best, 4).tolist() == [1, 4, 5, 2]        # NaN lowest, then -0 = +0 by row, then 0.1 by row
    f = np.concatenate([R.unit_rows(3, 64, 11)] * 4)              # 3 distinct rows, 12 in all: k = 5 forces two empty clusters
    r = R.kmeans(f, 5, iters=6, init="random", seed=1)
    assert r["reseeded"] >= 2 and r["iterations"] <= 6 and r["changed"] == 0 and (r["counts"] == 0).sum() >= 2
    assert sorted(r["counts"][r["counts"] > 0].tolist()) == [4, 4, 4]


# ------------------------------------------------------------------------------------------------------------------ input conditions
def test_planted_mixture_decisions_have_margin():
    """tests/test_cluster_path_gpu.py: every assignment of every iteration and every pick of the initialisation is decided by more than
    100 delta in float64; the clustering recovers the planted partition."""
    f, label = R.planted_mixture()
    r = R.kmeans(f, 8)
    lim = 100 * R.DELTA[64]
    print(f"planted mixture: iteration margins {r['margins']}, least init margin {r['init_margins'].min():.3e}, 100 delta {lim:.3e}")
    assert min(r["margins"]) > lim and r["init_margins"].min() > lim
    assert r["changed"] == 0 and r["reseeded"] == 0 and r["iterations"] < 20
    relabel = {}
    for a, l in zip(r["assign"].tolist(), label.tolist()):
        assert relabel.setdefault(a, l) == l
    assert len(set(relabel.values())) == 8
    assert all(b >= a - R.DELTA[64] for a, b in zip(r["objective"], r["objective"][1:]))


def test_pick_inputs_have_margin():
    rows, sim, margins = R.farthest_first(R.pick_rows(), 16, seed=R.PICK_SEED)
    print(f"picks: least margin {margins.min():.3e}, 100 delta {100 * R.DELTA[64]:.3e}")
    assert margins.min() > 100 * R.DELTA[64] and len(set(rows.tolist())) == 16


def test_tolerances_are_under_their_caps():
    for E, d in R.DELTA.items():
        assert 0 < d <= R.DELTA_CAP[E]
    assert 0 < R.CENTROID_TOL < 1e-4


# ------------------------------------------------------------------------------------------------------------------ seeded defects
@pytest.fixture(scope="module")
def case():
    f, c = R.unit_rows(100, 64, 20), R.unit_rows(30, 64, 21)
    c[29] = c[0]
    c[12] = c[5]
    f[:4] = c[[0, 5, 0, 5]]                                        # rows whose best centre has a copy
    return f, c


def test_checks_accept_the_reference(case):
    f, c = case
    best, idx, _ = R.assign(f, c)
    R.check_assign(best.astype(np.float32), idx, f, c, R.DELTA[64])
    R.check_same_bits((best, idx), (best, idx))


def test_defect_tie_to_the_highest_index_is_rejected(case):
    f, c = case
    S = R.scores64(f, c)
    idx = S.shape[1] - 1 - S[:, ::-1].argmax(1)                    # the LAST of equal maxima
    with pytest.raises(AssertionError, match="a copy of the chosen centre has a lower index"):
        R.check_assign(S.max(1), idx, f, c, R.DELTA[64])


def test_defect_merge_that_ignores_the_state_is_rejected(case):
    f, c = case
    one = R.assign(f, c)
    for cut in (1, 16, 17, 29):
        ignoring = R.assign(f, c[cut:], c0=cut)                    # what a merge that drops the state returns
        with pytest.raises(AssertionError, match="differs"):
            R.check_same_bits(one, ignoring[:2])


def test_defect_wrong_score_or_wrong_centre_is_rejected(case):
    f, c = case
    best, idx, _ = R.assign(f, c)
    off = best.copy()
    off[50] += 3 * R.DELTA[64]
    with pytest.raises(AssertionError, match="best against float64"):
        R.check_assign(off, idx, f, c, R.DELTA[64])
    S = R.scores64(f, c)
    wrong = idx.copy()
    wrong[60] = np.argsort(S[60])[-2]
    with pytest.raises(AssertionError, match="not the nearest"):
        R.check_assign(S[np.arange(100), wrong], wrong, f, c, R.DELTA[64])


def test_defect_unstable_member_order_is_rejected():
    a = np.random.default_rng(22).integers(-1, 5, size=300)
    counts, offsets, members, outside = R.group(a, 4)
    R.check_group(counts, offsets, members, outside, a, 4)
    swapped = members.copy()
    lo = offsets[2]
    swapped[[lo, lo + 1]] = swapped[[lo + 1, lo]]                  # the same set per cluster, one pair out of order
    with pytest.raises(AssertionError, match="do not ascend"):
        R.check_group(counts, offsets, swapped, outside, a, 4)
    with pytest.raises(AssertionError, match="outside"):
        R.check_group(counts, offsets, members, outside + 1, a, 4)


def _centroid_inputs():
    a = np.array([0] * 30 + [2] * 50 + [3] * 2)
    f = R.unit_rows(len(a), 64, 23)
    f[81] = -f[80]                                                 # cluster 3 cancels; cluster 1 is empty
    best = np.random.default_rng(24).random(len(a))
    best[[35, 60]] = 2.0                                           # a tie for cluster 2's medoid
    old = R.unit_rows(4, 64, 25)
    return a, f, best, old, R.group(a, 4)


def test_defect_medoid_by_lowest_best_is_rejected():
    a, f, best, old, (counts, offsets, members, _) = _centroid_inputs()
    cen, norm, med, _ = R.centroids(f, best, counts, offsets, members, old)
    R.check_centroids(cen.astype(np.float32), norm, med, f, best, counts, offsets, members, old, R.CENTROID_TOL)
    low = med.copy()
    low[0] = int(np.argmin(best[:30]))
    with pytest.raises(AssertionError, match="medoid"):
        R.check_centroids(cen.astype(np.float32), norm, low, f, best, counts, offsets, members, old, R.CENTROID_TOL)
    high_row = med.copy()
    high_row[2] = 60                                               # the tie broken towards the higher row
    with pytest.raises(AssertionError, match="medoid"):
        R.check_centroids(cen.astype(np.float32), norm, high_row, f, best, counts, offsets, members, old, R.CENTROID_TOL)


def test_defect_centre_written_for_an_empty_cluster_is_rejected():
    a, f, best, old, (counts, offsets, members, _) = _centroid_inputs()
    cen, norm, med, _ = R.centroids(f, best, counts, offsets, members, old)
    for c in (1, 3):                                               # the empty cluster, the cancelled one
        bad = cen.astype(np.float32)
        bad[c] = 0.0
        with pytest.raises(AssertionError, match=f"the centre of cluster {c} was written"):
            R.check_centroids(bad, norm, med, f, best, counts, offsets, members, old, R.CENTROID_TOL)
    off = cen.astype(np.float32)
    off[2, 7] += 3 * R.CENTROID_TOL
    with pytest.raises(AssertionError):
        R.check_centroids(off, norm, med, f, best, counts, offsets, members, old, R.CENTROID_TOL)
