"""spmm_leader_round / spmm_leader_finish (csrc/neighbors.hip) on hand-built neighbour lists, integer-exact against the sequential algorithm
and the model of the rounds in tests/butina_reference.py.  One wave64 per row strides the row's list: the star's hub crosses the 64-lane
stride 79 times.  States and leaders sit in sentinel-padded buffers."""
import numpy as np
import pytest
import torch

import butina_reference as B

pytestmark = pytest.mark.gpu

PAD = 16
S_PAD = 99


def _dev(lists):
    return tuple(torch.from_numpy(a).cuda() for a in B.csr(lists))


def _padded(n, fill=S_PAD):
    buf = torch.full((n + 2 * PAD,), fill, dtype=torch.int32, device="cuda")
    return buf, buf[PAD:PAD + n]


def _intact(buf, n, fill=S_PAD):
    return bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all())


def _rounds(lists, by_count, sync_every=1, check_each=False):
    """Rounds from the all-open state, the open count read every `sync_every` rounds -> (state, rounds) as numpy / int."""
    from spmm_amd import ops
    counts, offsets, nbr = _dev(lists)
    n = len(lists)
    bufs = [_padded(n), _padded(n)]
    bufs[0][1].zero_()
    cur, done, host_state = 0, 0, np.zeros(n, dtype=np.int64)
    while True:
        opened = torch.zeros(sync_every, dtype=torch.int32, device="cuda")
        for r in range(sync_every):
            ops.leader_round(counts, offsets, nbr, bufs[cur][1], bufs[1 - cur][1], opened[r:r + 1], by_count=by_count)
            cur = 1 - cur
            if check_each:
                torch.cuda.synchronize()
                out = bufs[cur][1].cpu().numpy()
                B.check_round(out, int(opened[r]), lists, by_count, host_state, f"in round {done + r + 1}")
                host_state = out
        host = opened.tolist()
        assert _intact(bufs[0][0], n) and _intact(bufs[1][0], n), "state written outside its rows"
        for r in range(sync_every):
            if host[r] == 0:
                return bufs[cur][1].cpu().numpy(), done + r + 1
        done += sync_every
        assert done <= n + sync_every, "the rounds do not end"


def _finish(lists, by_count, state):
    from spmm_amd import ops
    counts, offsets, nbr = _dev(lists)
    n = len(lists)
    buf, view = _padded(n, -5)
    st = torch.from_numpy(np.asarray(state, dtype=np.int32)).cuda()
    for _ in range(2):
        ops.leader_finish(counts, offsets, nbr, st, view, by_count=by_count)
    torch.cuda.synchronize()
    assert _intact(buf, n, -5), "leader written outside its rows"
    return view.cpu().numpy()


def _whole(lists, by_count, want_rounds=None, check_each=False):
    state, n_rounds = _rounds(lists, by_count, check_each=check_each)
    model, model_rounds, _ = B.rounds(lists, by_count)
    assert np.array_equal(state, model) and n_rounds == model_rounds
    if want_rounds is not None:
        assert n_rounds == want_rounds
    leader = _finish(lists, by_count, state)
    B.check_leaders(leader, lists, by_count)
    return state, leader, n_rounds


def test_path_under_row_priority_takes_a_round_per_row():
    state, leader, _ = _whole(B.path(300), False, want_rounds=300)
    assert np.array_equal(np.nonzero(state == 1)[0], np.arange(0, 300, 2)), "the leaders are the even rows"
    assert np.array_equal(leader, np.arange(300) // 2 * 2)


def test_path_under_count_priority():
    state, leader, n_rounds = _whole(B.path(300), True)
    assert leader[:4].tolist() == [1, 1, 1, 3] and n_rounds < 300


@pytest.mark.parametrize("by_count", [False, True])
def test_star_crosses_the_lane_stride(by_count):
    state, leader, _ = _whole(B.star(5000), by_count, want_rounds=2, check_each=True)
    assert bool((leader == 0).all())
    hub_last = [[5000]] * 5000 + [list(range(5000))]
    state, leader, _ = _whole(hub_last, by_count, check_each=True)
    assert bool((leader == 5000).all()) if by_count else leader.tolist() == list(range(5000)) + [0]


@pytest.mark.parametrize("by_count", [False, True])
def test_complete_and_empty_graphs(by_count):
    state, leader, _ = _whole(B.complete(100), by_count, want_rounds=2, check_each=True)
    assert bool((leader == 0).all())
    state, leader, _ = _whole([[] for _ in range(70)], by_count, want_rounds=1, check_each=True)
    assert np.array_equal(leader, np.arange(70))


@pytest.mark.parametrize("by_count", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_random_graphs_with_equal_counts(n, by_count):
    lists = B.random_graph(n, {1: 0.5, 63: 0.1, 64: 0.1, 65: 0.1, 1000: 0.01}[n], seed=n)
    if n >= 63:
        assert len({len(l) for l in lists}) < n, "no two rows of equal count"
    _whole(lists, by_count, check_each=n <= 65)


@pytest.mark.parametrize("by_count", [False, True])
def test_double_buffering_any_sync_every_ends_in_the_same_state(by_count):
    lists = B.random_graph(300, 0.02, seed=9) if by_count else B.path(41)
    one, n_rounds = _rounds(lists, by_count, sync_every=1)
    for every in (3, 7):
        state, again = _rounds(lists, by_count, sync_every=every)
        assert np.array_equal(state, one) and again == n_rounds, f"sync_every={every}"


def test_finish_binds_a_member_to_its_highest_priority_leader():
    lists = [[2], [2], [0, 1]]                                                  # row 2 is a neighbour of the leaders 0 and 1
    assert _finish(lists, False, [1, 1, 2]).tolist() == [0, 1, 0]
    lists = [[3], [2, 3, 4], [1], [0, 1], [1]]                                  # counts 1 3 1 2 1: row 1 leads; row 3 is claimed by 1, not by 0
    state, leader, _ = _whole(lists, True)
    assert state.tolist() == [1, 1, 2, 2, 2] and leader.tolist() == [0, 1, 1, 1, 1]
    assert _finish(lists, True, [0, 1, 2, 0, 2]).tolist() == [-1, 1, 1, 1, 1], "a row with no leader among its neighbours gets -1"
