"""spmm_amd.cluster's threshold clustering on the GPU -- neighbours, leaders, dedup and the cluster.py driver -- against
tests/butina_reference.py and against its own tensor-library form (engine=False)."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

import butina_reference as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TENSORS = ("leader", "cluster", "leaders", "counts", "offsets", "members", "n_neighbours")


def _same_fields(a, b, E, what):
    for name in TENSORS:
        x, y = getattr(a, name).cpu(), getattr(b, name).cpu()
        assert x.dtype == y.dtype and torch.equal(x, y), f"{name} differs {what}"
    assert (a.rounds, a.threshold, a.order, a.pairs) == (b.rounds, b.threshold, b.order, b.pairs), what
    x, y = a.cosine_to_leader.cpu().numpy(), b.cosine_to_leader.cpu().numpy()
    assert x.dtype == y.dtype == np.float32 and np.array_equal(np.isnan(x), np.isnan(y))
    ok = ~np.isnan(x)
    assert np.abs(x[ok].astype(np.float64) - y[ok]).max() <= B.DELTA_CAP[E], f"cosine_to_leader (an fp32 dot product on either device) {what}"


def test_planted_mixture_is_recovered_exactly():
    """12 groups of 5 .. 120 rows, within-group cosine above 0.9, between groups below 0.3 (asserted by test_butina_reference_cpu.py), threshold
    0.6: the groups come back exactly, each led by its lowest row, numbered by size with ties by leader row."""
    from spmm_amd import cluster as C
    f, label = B.planted_groups()
    res = C.leaders(torch.from_numpy(f).cuda(), B.MIX_THRESHOLD)
    leader, cluster = res.leader.cpu().numpy(), res.cluster.cpu().numpy()
    lowest = {g: int(np.nonzero(label == g)[0][0]) for g in range(len(B.GROUP_SIZES))}
    assert np.array_equal(leader, [lowest[g] for g in label]), "every group is led by its lowest row"
    order = sorted(range(len(B.GROUP_SIZES)), key=lambda g: (-B.GROUP_SIZES[g], lowest[g]))
    assert res.leaders.cpu().tolist() == [lowest[g] for g in order]
    assert np.array_equal(cluster, [order.index(g) for g in label])
    assert res.counts.cpu().tolist() == [B.GROUP_SIZES[g] for g in order]
    assert np.array_equal(res.n_neighbours.cpu().numpy(), [B.GROUP_SIZES[g] - 1 for g in label])
    for c, g in enumerate(order):
        seg = res.members[int(res.offsets[c]):int(res.offsets[c + 1])].cpu().numpy()
        assert np.array_equal(seg, np.nonzero(label == g)[0])
    assert res.rounds == 2 and res.pairs == sum(s * (s - 1) for s in B.GROUP_SIZES)
    cos = res.cosine_to_leader.cpu().numpy()
    assert bool((cos[leader == np.arange(len(label))] == 1.0).all()) and cos.min() > 0.9


@pytest.mark.parametrize("order", ["count", "row"])
@pytest.mark.parametrize("E", [64, 256])
def test_engine_equals_the_tensor_form(E, order):
    """Picked-threshold random inputs (copies, a NaN row, a zero row): every pair is decided alike in fp32 and float64, so the two forms agree
    field for field; so do two runs, other chunkings and other sync_every."""
    from spmm_amd import cluster as C
    x, S, t, margin = B.range_input(1000, E)
    assert margin >= B.DELTA[E]
    f = torch.from_numpy(x).cuda()
    res = C.leaders(f, t, order=order)
    ref = C.leaders(torch.from_numpy(x), t, order=order, engine=False)
    _same_fields(res, ref, E, "between the engine and the tensor form")
    lists = B.neighbour_lists(S, t)
    B.check_leaders(res.leader.cpu().numpy(), lists, order == "count")
    again = C.leaders(f, t, order=order, sync_every=3, chunk=300)
    _same_fields(res, again, E, "between two runs (sync_every 3, columns in chunks of 300)")
    assert torch.equal(res.cosine_to_leader, again.cosine_to_leader), "two runs differ in their bytes"
    got = C.neighbours(f, t, chunk=129)
    B.check_lists(*(a.cpu().numpy() for a in got), lists)
    csr = C.leaders(got, order=order, sync_every=7)
    assert torch.equal(csr.leader, res.leader) and csr.rounds == res.rounds and csr.cosine_to_leader is None


def test_dedup_keeps_the_first_of_each_set():
    from spmm_amd import cluster as C
    x, first = B.dedup_library()
    f = torch.from_numpy(x).cuda()
    keep = C.dedup(f, B.DEDUP_THRESHOLD)
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), first == np.arange(len(first)))
    assert np.array_equal(C.leaders(f, B.DEDUP_THRESHOLD, order="row").leader.cpu().numpy(), first)


def test_max_pairs_refuses_before_the_emit_pass_allocates(monkeypatch):
    from spmm_amd import cluster as C
    from spmm_amd import ops
    x, S, t, _ = B.range_input(256, 64)
    M = sum(len(l) for l in B.neighbour_lists(S, t))
    calls = []
    real = ops.sim_range

    def spy(*a, **k):
        calls.append(k.get("nbr") is not None)
        return real(*a, **k)

    monkeypatch.setattr(ops, "sim_range", spy)
    with pytest.raises(ValueError, match=rf"{M} neighbour entries at threshold .* exceed max_pairs={M - 1} \(--max_pairs\)"):
        C.neighbours(torch.from_numpy(x).cuda(), t, max_pairs=M - 1)
    assert calls == [False], "the count pass only: no emit launch, no list"
    calls.clear()
    assert C.neighbours(torch.from_numpy(x).cuda(), t, max_pairs=M)[2].numel() == M and calls == [False, True]


def _rows(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


def test_driver_through_the_tiny_model(tmp_path, capsys):
    """cluster.py --synthetic 200 --tiny --threshold T / --dedup T: every line in exactly one cluster, each cluster's is_medoid row its leader,
    every member within T - DELTA of its leader, no two leaders T + DELTA similar.  A seeded model's features are no random directions --
    its pair cosines crowd within 3e-4 below 1, the widest gap among them is 2e-7 -- so no threshold keeps every pair a DELTA away and the
    float64 side is held to DELTA; the leaders are integer-exact against the sequential algorithm on the engine's own neighbour list."""
    sys.path.insert(0, ROOT)
    import cluster
    from spmm_amd import cluster as C
    from spmm_amd import retrieve as Rt
    base = ["--synthetic", "200", "--tiny", "--seed", "1"]
    idx = tmp_path / "lib.idx"
    cluster.main(cluster.parse_args(base + ["--k", "3", "--output", str(tmp_path / "k.csv"), "--save_index", str(idx)]))
    index = Rt.MoleculeIndex.load(str(idx), device=torch.device("cuda"))
    feats = index.feats.cpu().numpy()
    E = feats.shape[1]
    S = B.cosines64(feats)
    T = float(np.float32(np.quantile(B.pair_values(S), 0.9)))
    delta = B.DELTA[E]
    lists = B.uncsr(*(a.cpu().numpy() for a in C.neighbours(index, T)))
    sure, maybe = B.neighbour_lists(S, T + delta), B.neighbour_lists(S, T - delta)
    assert B.symmetric(lists) and all(set(a) <= set(l) <= set(b) for a, l, b in zip(sure, lists, maybe)), "the list against float64"
    assert sum(map(len, lists)) > 200
    for order in ("count", "row"):
        out, meds = tmp_path / f"c_{order}.csv", tmp_path / f"m_{order}.csv"
        cluster.main(cluster.parse_args(base + ["--threshold", repr(T), "--order", order, "--output", str(out), "--medoids", str(meds)]))
        rows = _rows(out)
        assert rows[0] == cluster.LEADER_HEADER and [int(r[0]) for r in rows[1:]] == list(range(1, 201))
        cl = np.array([int(r[2]) for r in rows[1:]])
        K = cl.max() + 1
        assert cl.min() == 0 and set(cl.tolist()) == set(range(K)), "every line is in exactly one cluster"
        lead_of = {}
        for i, r in enumerate(rows[1:]):
            if r[4] == "1":
                assert cl[i] not in lead_of, "two leaders in one cluster"
                lead_of[cl[i]] = i
        assert sorted(lead_of) == list(range(K)), "one is_medoid row per cluster"
        for i, r in enumerate(rows[1:]):
            l = lead_of[cl[i]]
            assert l == i or S[i, l] >= T - delta, (i, l, S[i, l])
            assert abs(float(r[3]) - (1.0 if l == i else S[i, l])) <= B.DELTA_CAP[E]
            assert int(r[5]) == len(lists[i])
        ls = sorted(lead_of.values())
        sub = S[np.ix_(ls, ls)] - 2 * np.eye(len(ls))
        assert sub.max() < T + delta, "two leaders within the threshold"
        B.check_leaders([lead_of[c] for c in cl], lists, order == "count")
        m = _rows(meds)
        assert m[0] == cluster.MEDOID_HEADER and len(m) == K + 1 and [int(r[2]) - 1 for r in m[1:]] == [lead_of[c] for c in range(K)]
        assert [int(r[1]) for r in m[1:]] == [int((cl == c).sum()) for c in range(K)]
    uniq = tmp_path / "u.csv"
    capsys.readouterr()
    cluster.main(cluster.parse_args(base + ["--dedup", repr(T), "--output", str(uniq)]))
    u = _rows(uniq)
    want = B.sequential(lists, False)
    kept = np.nonzero(want == np.arange(200))[0]
    assert u[0] == cluster.DEDUP_HEADER and [int(r[0]) - 1 for r in u[1:]] == kept.tolist()
    assert (S[np.ix_(kept, kept)] - 2 * np.eye(len(kept))).max() < T + delta, "two kept lines within the threshold"
    text = capsys.readouterr().out
    assert f"{200 - len(kept)} of 200 lines dropped" in text
    for i in np.nonzero(want != np.arange(200))[0]:
        assert "line %-8d dropped: a duplicate of line %d" % (i + 1, want[i] + 1) in text
        assert want[i] < i and S[i, want[i]] >= T - delta
