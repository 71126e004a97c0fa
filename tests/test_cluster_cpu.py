"""spmm_amd/cluster.py's tensor-op forms (engine=False: float64 scores, CPU tensors) against tests/kmeans_reference.py, the re-seeding
order, and the shapes and dtypes of a Clustering.  No GPU, no kernel."""
import numpy as np
import pytest
import torch

import kmeans_reference as R
from spmm_amd import cluster as C


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def test_assign_matches_the_reference():
    f, c = R.unit_rows(300, 64, 1), R.unit_rows(40, 64, 2)
    c[33] = c[4]
    f[7] = c[4]
    f[8] = np.nan
    f[9] = 0.0
    best, idx = C.assign(_t(f), _t(c), engine=False)
    rb, ri, _ = R.assign(f, c)
    assert best.dtype == torch.float32 and idx.dtype == torch.int32 and best.shape == idx.shape == (300,)
    assert np.array_equal(idx.numpy(), ri) and idx[7] == 4 and idx[8] == 0 and idx[9] == 0
    assert np.array_equal(best.numpy(), rb.astype(np.float32), equal_nan=True)
    assert torch.isnan(best[8]) and best[9] == 0 and not np.signbit(best[9].item())
    with pytest.raises(ValueError, match="do not match"):
        C.assign(_t(f), _t(R.unit_rows(4, 128, 3)), engine=False)


def test_merge_rule_matches_the_reference_order():
    best = torch.tensor([0.5, 0.5, float("nan"), float("-inf"), -0.0, 0.2, float("nan")])
    idx = torch.tensor([3, 3, 2, -1, 1, 4, 5], dtype=torch.int32)
    nb = torch.tensor([0.5, 0.5, -5.0, float("nan"), 0.0, 0.1, float("nan")])
    ni = torch.tensor([2, 9, 7, 6, 0, 0, 1], dtype=torch.int32)
    b, i = C._merge_tensor(best, idx, nb, ni)
    assert i.tolist() == [2, 3, 7, 6, 0, 4, 1]
    for j in range(7):
        want = R.better(float(nb[j]), int(ni[j]), float(best[j]), int(idx[j]))
        assert (int(i[j]) == int(ni[j])) == want


def test_pick_diverse_matches_the_reference():
    f = R.pick_rows()
    rows, sim = C.pick_diverse(_t(f), 16, seed=R.PICK_SEED, engine=False)
    rr, rs, _ = R.farthest_first(f, 16, seed=R.PICK_SEED)
    assert rows.dtype == torch.int64 and sim.dtype == torch.float32 and rows.shape == sim.shape == (16,)
    assert rows.tolist() == rr.tolist() and np.allclose(sim.numpy()[1:], rs[1:], atol=1e-6) and sim[0] == float("-inf")
    assert C.pick_diverse(_t(f), 3, first=77, engine=False)[0][0] == 77
    assert C.pick_diverse(_t(f), 3, seed=9, engine=False)[0][0] == R.first_row(500, None, 9) == C.first_row(500, None, 9)
    dup = np.concatenate([f[:6], f[:6]])
    rows = C.pick_diverse(_t(dup), 6, first=8, engine=False)[0]
    assert sorted((rows % 6).tolist()) == list(range(6))
    with pytest.raises(ValueError, match=r"n=0 must be in \[1, 500\]"):
        C.pick_diverse(_t(f), 0, engine=False)
    with pytest.raises(ValueError, match="first=500"):
        C.pick_diverse(_t(f), 2, first=500, engine=False)


@pytest.fixture(scope="module")
def planted():
    f, label = R.planted_mixture()
    return f, label, R.kmeans(f, 8)


@pytest.mark.parametrize("sync_every", [1, 4])
def test_kmeans_matches_the_reference(planted, sync_every):
    f, label, ref = planted
    res = C.kmeans(_t(f), 8, sync_every=sync_every, engine=False)
    assert res.iterations == ref["iterations"] and res.changed == 0 and res.reseeded == 0
    assert np.array_equal(res.assign.numpy(), ref["assign"]) and np.array_equal(res.counts.numpy(), ref["counts"])
    assert np.array_equal(res.offsets.numpy(), ref["offsets"]) and np.array_equal(res.members.numpy(), ref["members"])
    assert np.array_equal(res.medoid.numpy(), ref["medoid"])
    assert np.allclose(res.centres.numpy(), ref["centres"], atol=1e-6) and np.allclose(res.objective, ref["objective"], atol=1e-3)
    assert np.allclose(res.best.numpy(), ref["best"], atol=1e-6)


def test_clustering_fields(planted):
    f, _, _ = planted
    N, E, k = f.shape[0], f.shape[1], 8
    res = C.kmeans(_t(f), k, iters=3, init="random", seed=2, engine=False)
    want = dict(centres=((k, E), torch.float32), assign=((N,), torch.int32), best=((N,), torch.float32), counts=((k,), torch.int32),
                offsets=((k + 1,), torch.int64), members=((N,), torch.int32), medoid=((k,), torch.int32))
    for name, (shape, dtype) in want.items():
        t = getattr(res, name)
        assert tuple(t.shape) == shape and t.dtype == dtype, name
    assert isinstance(res.objective, list) and len(res.objective) == res.iterations <= 3 and all(isinstance(o, float) for o in res.objective)
    assert isinstance(res.iterations, int) and isinstance(res.reseeded, int) and isinstance(res.changed, int)
    assert torch.allclose(res.centres.norm(dim=1), torch.ones(k), atol=1e-5)
    ref = R.kmeans(f, k, iters=3, init="random", seed=2)
    assert np.array_equal(res.assign.numpy(), ref["assign"]) and res.iterations == ref["iterations"]
    with pytest.raises(ValueError, match=r"k=0 must be in \[1, 2000\]"):
        C.kmeans(_t(f), 0, engine=False)
    with pytest.raises(ValueError, match="init='nearest'"):
        C.kmeans(_t(f), 2, init="nearest", engine=False)


def test_reseeding_order_and_forced_empties():
    """More clusters than distinct rows: the empty clusters take the rows with the lowest best, in order, every iteration; the run ends."""
    f = np.concatenate([R.unit_rows(3, 64, 11)] * 4)
    res = C.kmeans(_t(f), 5, iters=6, init="random", seed=1, sync_every=2, engine=False)
    assert res.reseeded >= 2 and res.iterations <= 6 and res.changed == 0
    assert sorted(res.counts[res.counts > 0].tolist()) == [4, 4, 4] and int((res.medoid < 0).sum()) == 2
    # one iteration against the rule applied to its own best (which of two rows that both sit on their centre is served worse is
    # decided in the last bit of a score, so the float64 reference is not asked)
    centres = _t(f[[0, 1, 0, 1, 0]].copy())                        # group 2 has no centre; centres 2, 3, 4 are copies and stay empty
    step = C._iteration(_t(f), centres, torch.full((12,), -1, dtype=torch.int32), 4096, False)
    assert sorted(step["counts"].tolist()) == [0, 0, 0, 4, 8] and step["stats"].tolist()[:2] == [12.0, 3.0]
    want = R.reseed_rows(step["best"].numpy(), 3)
    assert torch.equal(step["centres"][2:], _t(f)[want]) and set(want.tolist()) <= {2, 5, 8, 11}
    # the order itself: NaN lowest, -0 = +0 by row, then ascending, ties to the lowest row
    best = torch.tensor([0.5, float("nan"), 0.1, 0.1, -0.0, 0.0, 0.9])
    rows = _t(R.unit_rows(7, 64, 12))
    centres = _t(R.unit_rows(6, 64, 13))
    bad = torch.tensor([False, True, True, False, True, True])
    new = C._reseed(rows, best, bad, centres)
    want = R.reseed_rows(best.numpy(), 4).tolist()
    assert want == [1, 4, 5, 2]
    assert torch.equal(new[[1, 2, 4, 5]], rows[want]) and torch.equal(new[[0, 3]], centres[[0, 3]])


def test_takes_an_index_object():
    class Index:
        feats = _t(R.unit_rows(50, 64, 14))
    rows, _ = C.pick_diverse(Index(), 4, first=0, engine=False)
    assert rows[0] == 0 and len(set(rows.tolist())) == 4
    with pytest.raises(TypeError, match="MoleculeIndex or an"):
        C.pick_diverse([1, 2, 3], 2, engine=False)
