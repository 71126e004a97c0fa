"""spmm_amd.cluster's threshold clustering in its tensor-library form (engine=False, CPU tensors) against tests/butina_reference.py: the
neighbour lists, the LeaderClustering fields, the cluster numbering, dedup and the max_pairs refusal."""
import numpy as np
import pytest
import torch

import butina_reference as B
from spmm_amd import cluster as C


@pytest.fixture(scope="module")
def small():
    f, S, t, _ = B.range_input(255, 64)
    return torch.from_numpy(f), B.neighbour_lists(S, t), t


def test_neighbours_tensor_form_against_the_brute_force_lists(small):
    f, want, t = small
    counts, offsets, nbr = C.neighbours(f, t, engine=False)
    assert counts.dtype == torch.int32 and offsets.dtype == torch.int64 and nbr.dtype == torch.int32
    assert offsets.numel() == f.shape[0] + 1 and int(offsets[-1]) == nbr.numel() == sum(len(l) for l in want)
    B.check_lists(counts.numpy(), offsets.numpy(), nbr.numpy(), want)
    assert B.symmetric(B.uncsr(counts.numpy(), offsets.numpy(), nbr.numpy()))


@pytest.mark.parametrize("order", ["count", "row"])
def test_leader_clustering_fields(small, order):
    f, lists, t = small
    by_count = order == "count"
    res = C.leaders(f, t, order=order, engine=False)
    N = f.shape[0]
    B.check_leaders(res.leader.numpy(), lists, by_count)
    rows, cluster = B.numbering(res.leader.numpy(), [len(l) for l in lists], by_count)
    assert res.leaders.dtype == torch.int64 and np.array_equal(res.leaders.numpy(), rows)
    assert res.cluster.dtype == torch.int32 and np.array_equal(res.cluster.numpy(), cluster)
    K = len(rows)
    assert res.counts.numel() == K and res.offsets.numel() == K + 1 and res.members.numel() == N and int(res.counts.sum()) == N
    for c in range(K):
        seg = res.members[int(res.offsets[c]):int(res.offsets[c + 1])].numpy()
        assert np.array_equal(seg, np.nonzero(cluster == c)[0]), f"members of cluster {c}"
    assert np.array_equal(res.n_neighbours.numpy(), [len(l) for l in lists])
    assert res.pairs == sum(len(l) for l in lists) and res.order == order and res.threshold == t
    assert res.rounds == B.rounds(lists, by_count)[1], "rounds of the parallel rule, from the sequential walk"
    cos = res.cosine_to_leader.numpy()
    lead = res.leader.numpy()
    assert cos.dtype == np.float32 and bool((cos[lead == np.arange(N)] == 1.0).all()), "a leader's cosine is 1.0 (the NaN row's too)"
    mem = np.nonzero(lead != np.arange(N))[0]
    S = B.cosines64(f.numpy())
    assert np.abs(cos[mem] - S[mem, lead[mem]]).max() <= B.DELTA_CAP[64]
    assert bool((cos[mem] >= t - B.DELTA_CAP[64]).all())
    if by_count:
        nn = res.n_neighbours.numpy()[rows]
        assert bool((np.diff(nn) <= 0).all()) and nn[0] == max(len(l) for l in lists), "cluster 0 is the most populated neighbourhood"


def test_leaders_take_a_neighbour_list():
    lists = B.random_graph(120, 0.05, seed=4)
    counts, offsets, nbr = (torch.from_numpy(a) for a in B.csr(lists))
    for order in ("count", "row"):
        res = C.leaders((counts, offsets, nbr), order=order, engine=False)
        B.check_leaders(res.leader.numpy(), lists, order == "count")
        assert res.cosine_to_leader is None and res.threshold is None
        assert res.rounds == B.rounds(lists, order == "count")[1]


def test_the_numbering_breaks_equal_counts_by_the_lower_leader():
    lists = B.complete(3) + [[j + 3 for j in l] for l in B.complete(3)] + [[7], [6]]     # two triangles and a pair
    counts, offsets, nbr = (torch.from_numpy(a) for a in B.csr(lists))
    res = C.leaders((counts, offsets, nbr), order="count", engine=False)
    assert res.leaders.tolist() == [0, 3, 6] and res.cluster.tolist() == [0, 0, 0, 1, 1, 1, 2, 2] and res.counts.tolist() == [3, 3, 2]


def test_dedup_keeps_first_occurrences():
    f, first = B.dedup_library()
    keep = C.dedup(torch.from_numpy(f), B.DEDUP_THRESHOLD, engine=False)
    assert keep.dtype == torch.bool and np.array_equal(keep.numpy(), first == np.arange(len(first)))
    res = C.leaders(torch.from_numpy(f), B.DEDUP_THRESHOLD, order="row", engine=False)
    assert np.array_equal(res.leader.numpy(), first), "every copy is folded into its first occurrence"


def test_max_pairs_refusal_names_the_size(small):
    f, lists, t = small
    M = sum(len(l) for l in lists)
    with pytest.raises(ValueError, match=rf"{M} neighbour entries at threshold .* exceed max_pairs={M - 1} \(--max_pairs\)"):
        C.neighbours(f, t, max_pairs=M - 1, engine=False)
    assert C.neighbours(f, t, max_pairs=M, engine=False)[2].numel() == M


def test_bad_arguments():
    f = torch.from_numpy(B.range_input(255, 64)[0])
    with pytest.raises(ValueError, match="order="):
        C.leaders(f, 0.5, order="size", engine=False)
    with pytest.raises(ValueError, match="need a threshold"):
        C.leaders(f, engine=False)
    with pytest.raises(ValueError, match="NaN"):
        C.neighbours(f, float("nan"), engine=False)
    empty = C.leaders(torch.zeros(0, 64), 0.5, engine=False)
    assert empty.leaders.numel() == 0 and empty.rounds == 0 and empty.pairs == 0
