"""tests/butina_reference.py checked against itself: the model of the parallel rounds and the finish rule give the sequential algorithm's
leaders; the threshold picker's margins hold on every input the GPU tests use; every check the GPU tests apply rejects a seeded defect."""
import numpy as np
import pytest

import butina_reference as B

GRAPHS = [(n, d, s) for s, (n, d) in enumerate([(1, 0.5), (2, 0.8), (3, 0.5), (7, 0.3), (16, 0.2), (33, 0.1), (59, 0.05), (64, 0.02), (100, 0.8),
                                                (150, 0.05), (200, 0.02), (200, 0.1)])]


def _agree(lists, by_count, want_rounds=None):
    assert B.symmetric(lists)
    want = B.sequential(lists, by_count)
    state, n_rounds, opens = B.rounds(lists, by_count, cap=len(lists) + 1)
    assert np.array_equal(state == 1, want == np.arange(len(lists))), "the leaders of the rounds are not the sequential algorithm's"
    assert np.array_equal(B.finish(lists, by_count, state), want), "finish binds a member to another leader"
    assert opens == sorted(opens, reverse=True) and opens[-1] == 0
    if want_rounds is not None:
        assert n_rounds == want_rounds
    return n_rounds


@pytest.mark.parametrize("by_count", [False, True])
@pytest.mark.parametrize("n,density,seed", GRAPHS)
def test_rounds_equal_the_sequential_algorithm_on_random_graphs(n, density, seed, by_count):
    lists = B.random_graph(n, density, seed)
    if n >= 16:
        counts = [len(l) for l in lists]
        assert len(set(counts)) < n, "no two rows of equal count"
    _agree(lists, by_count)


@pytest.mark.parametrize("by_count", [False, True])
def test_rounds_on_the_special_graphs(by_count):
    _agree(B.path(40), by_count, want_rounds=40 if not by_count else None)       # row priority: one row per round
    _agree(B.star(70), by_count, want_rounds=2 if by_count else 2)
    _agree(B.complete(30), by_count, want_rounds=2)
    _agree([[] for _ in range(9)], by_count, want_rounds=1)
    two = B.path(5) + [[j + 5 for j in l] for l in B.complete(4)]                # two components
    _agree(two, by_count)
    assert B.sequential(B.path(6), False).tolist() == [0, 0, 2, 2, 4, 4]
    assert B.sequential(B.path(5), True).tolist() == [1, 1, 1, 3, 3]             # interior rows have two neighbours: 1 leads, then 3


def test_star_leader_depends_on_the_priority():
    assert B.sequential(B.star(5), True).tolist() == [0] * 6
    assert B.sequential(B.star(5), False).tolist() == [0] * 6
    shifted = [[5]] * 5 + [[0, 1, 2, 3, 4]]                                     # the hub is the LAST row
    assert B.sequential(shifted, True).tolist() == [5] * 6
    assert B.sequential(shifted, False).tolist() == [0, 1, 2, 3, 4, 0]


# ------------------------------------------------------------------------------------------------------------------ margins of the inputs
@pytest.mark.parametrize("n,E", B.RANGE_CASES)
def test_picked_thresholds_keep_every_pair_a_delta_away(n, E):
    f, S, t, margin = B.range_input(n, E)
    assert np.float32(t) == t and margin >= B.DELTA[E] and B.DELTA[E] <= B.DELTA_CAP[E]
    assert abs(t - B.RANGE_TARGET[E]) < 0.01
    lists = B.neighbour_lists(S, t)
    assert B.symmetric(lists) and lists[5] == [] and all(5 not in l for l in lists), "the NaN row has no neighbours and is nobody's"
    assert {0, 3, n - 1} - {0} <= set(lists[0]), "exact copies are neighbours"
    assert lists[7] == [] and sum(len(l) for l in lists) > 4 * n, "a non-trivial degree"


def test_planted_groups_margins():
    f, label = B.planted_groups()
    S = B.cosines64(f)
    same = label[:, None] == label[None, :]
    off = ~np.eye(len(label), dtype=bool)
    assert S[same & off].min() > 0.9 and S[~same].max() < 0.3
    assert min(B.GROUP_SIZES) == 5 and max(B.GROUP_SIZES) == 120 and len(B.GROUP_SIZES) == 12


def test_dedup_library_margins():
    f, first = B.dedup_library()
    S = B.cosines64(f)
    E = f.shape[1]
    n = len(first)
    assert (first != np.arange(n)).sum() >= 20 and (first <= np.arange(n)).all()
    for i in range(n):
        for j in range(i):
            if first[i] == first[j]:
                assert S[i, j] >= B.DEDUP_THRESHOLD + 100 * B.DELTA[E], (i, j, S[i, j])
            else:
                assert S[i, j] <= B.DEDUP_THRESHOLD - 100 * B.DELTA[E], (i, j, S[i, j])


def test_the_picker_refuses_what_it_cannot_separate():
    v = np.arange(0.0, 1.0, 1e-7)
    with pytest.raises(AssertionError, match="no gap"):
        B.pick_threshold(v, 0.5, B.DELTA[64])
    t, margin = B.pick_threshold(np.array([0.1, 0.2, 0.2 + 1e-7, 0.4]), 0.24, B.DELTA[64])
    assert 0.29 < t < 0.31 and margin > 0.09                                    # the gap nearest the target that is wide enough


# ------------------------------------------------------------------------------------------------------------------ seeded defects
S4 = np.array([[1.0, 0.5, 0.25, 0.75], [0.5, 1.0, 0.5, 0.0], [0.25, 0.5, 1.0, np.nan], [0.75, 0.0, np.nan, 1.0]])


def test_check_lists_rejects_a_kept_diagonal():
    want = B.neighbour_lists(S4, 0.5)
    assert want == [[1, 3], [0, 2], [1], [0]]
    B.check_lists(*B.csr(want), want)
    with pytest.raises(AssertionError, match="neighbours"):
        B.check_lists(*B.csr([sorted(l + [i]) for i, l in enumerate(want)]), want)


def test_check_lists_rejects_a_strict_compare():
    want = B.neighbour_lists(S4, 0.5)
    strict = [[j for j in range(4) if j != i and S4[i, j] > 0.5] for i in range(4)]
    assert strict != want
    with pytest.raises(AssertionError, match="neighbours"):
        B.check_lists(*B.csr(strict), want)


def test_check_lists_rejects_a_list_out_of_order():
    want = B.neighbour_lists(S4, 0.5)
    with pytest.raises(AssertionError, match="does not ascend"):
        B.check_lists(*B.csr([l[::-1] for l in want]), want)


def test_check_leaders_rejects_a_tie_to_the_higher_row():
    lists = B.path(4)                                                             # rows 1 and 2 tie with two neighbours each
    B.check_leaders(B.sequential(lists, True), lists, True)
    wrong = B.sequential(lists, True, tie_high=True)
    assert wrong.tolist() == [0, 2, 2, 2] and B.sequential(lists, True).tolist() == [1, 1, 1, 3]
    with pytest.raises(AssertionError, match="leader of row"):
        B.check_leaders(wrong, lists, True)


def test_check_leaders_rejects_a_member_bound_to_a_lower_priority_leader():
    lists = [[2], [2], [0, 1]]                                                    # row 2 is a neighbour of the leaders 0 and 1 (row priority)
    state, _, _ = B.rounds(lists, False)
    assert state.tolist() == [1, 1, 2]
    B.check_leaders(B.finish(lists, False, state), lists, False)
    with pytest.raises(AssertionError, match="leader of row"):
        B.check_leaders(B.finish(lists, False, state, lowest=True), lists, False)


def test_check_round_rejects_a_round_that_reads_its_own_output():
    lists = B.path(6)
    zero = np.zeros(6, dtype=np.int64)
    good, left = B.one_round(lists, False, zero)
    assert good.tolist() == [1, 0, 0, 0, 0, 0] and left == 5
    B.check_round(good, left, lists, False, zero)
    bad, bad_left = B.one_round(lists, False, zero, in_place=True)
    assert bad.tolist() == [1, 2, 1, 2, 1, 2]
    with pytest.raises(AssertionError, match="state after the round"):
        B.check_round(bad, bad_left, lists, False, zero)
    with pytest.raises(AssertionError, match="open rows"):
        B.check_round(good, left - 1, lists, False, zero)
