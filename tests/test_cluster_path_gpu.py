"""spmm_amd/cluster.py on the GPU -- kmeans, pick_diverse and the cluster.py driver -- against tests/kmeans_reference.py.

The planted-mixture and pick inputs are the ones tests/test_cluster_reference_cpu.py vets: every decision the float64 reference makes on
them has a margin above 100 delta, so the fp32 path must make the same decisions exactly."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

import kmeans_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture(scope="module")
def planted():
    f, label = R.planted_mixture()
    return f, label, R.kmeans(f, 8)


def _consistent(res, N, k):
    """members / offsets / counts / medoid against assign and best."""
    a, best = res.assign.cpu().numpy(), res.best.cpu().numpy()
    R.check_group(res.counts.cpu().numpy(), res.offsets.cpu().numpy(), res.members.cpu().numpy(), int(((a < 0) | (a >= k)).sum()), a, k)
    assert bool((res.members.cpu().numpy()[int(res.offsets[k]):] == -1).all())
    med = res.medoid.cpu().numpy()
    for c in range(k):
        rows = np.nonzero(a == c)[0]
        if len(rows) == 0:
            assert med[c] == -1
        else:
            assert a[med[c]] == c and best[med[c]] == best[rows].max() and med[c] == rows[best[rows] == best[rows].max()][0]


def test_planted_mixture(planted):
    from spmm_amd import cluster as C
    f, label, ref = planted
    res = C.kmeans(_d(f), 8, init="farthest")
    a = res.assign.cpu().numpy()
    assert np.array_equal(a, ref["assign"]), "the assignment differs from the float64 reference's"
    relabel = {}
    for x, l in zip(a.tolist(), label.tolist()):
        assert relabel.setdefault(x, l) == l, "a cluster mixes two planted directions"
    assert len(set(relabel.values())) == 8
    assert res.changed == 0 and res.iterations == ref["iterations"] < 20 and res.reseeded == 0
    print(f"objective {res.objective} reference {ref['objective']}")
    assert all(b >= x - R.DELTA[64] * len(f) for x, b in zip(res.objective, res.objective[1:]))      # (a sum over N rows, each within delta)
    per_row = R.DELTA[64] + 8 * R.CENTROID_TOL                     # the score's own error and the centre's (64 components, a unit row)
    assert np.allclose(res.objective, ref["objective"], atol=per_row * len(f))
    assert np.abs(res.best.cpu().numpy() - ref["best"]).max() <= per_row
    assert np.abs(res.centres.cpu().numpy() - ref["centres"]).max() <= R.CENTROID_TOL
    _consistent(res, len(f), 8)


def test_kmeans_is_deterministic_and_chunking_changes_nothing(planted):
    from spmm_amd import cluster as C
    f = _d(planted[0])
    a = C.kmeans(f, 8)
    for kw in (dict(), dict(chunk=3), dict(sync_every=1), dict(chunk=1, sync_every=7)):
        b = C.kmeans(f, 8, **kw)
        for name in ("centres", "assign", "best", "counts", "offsets", "members", "medoid"):
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (name, kw)
        assert a.objective == b.objective and a.iterations == b.iterations and a.reseeded == b.reseeded
    best, idx = C.assign(f, a.centres)
    for chunk in (1, 3, 5):
        b2, i2 = C.assign(f, a.centres, chunk=chunk)
        assert torch.equal(best.view(torch.int32), b2.view(torch.int32)) and torch.equal(idx, i2), chunk


def test_forced_empty_clusters_are_reseeded():
    """More clusters than distinct rows: two clusters are empty in every iteration; they take the rows with the lowest best (checked
    against the rule applied to the iteration's own best) and the run ends."""
    from spmm_amd import cluster as C
    f_h = np.concatenate([R.unit_rows(3, 64, 11)] * 4)
    f = _d(f_h)
    res = C.kmeans(f, 5, iters=6, init="random", seed=1, sync_every=2)
    assert res.reseeded >= 2 and res.iterations <= 6 and res.changed == 0
    assert sorted(res.counts[res.counts > 0].tolist()) == [4, 4, 4] and int((res.medoid < 0).sum()) == 2
    _consistent(res, 12, 5)
    centres = _d(f_h[[0, 1, 0, 1, 0]].copy())
    step = C._iteration(f, centres, torch.full((12,), -1, dtype=torch.int32, device="cuda"), 4096, True)
    assert sorted(step["counts"].tolist()) == [0, 0, 0, 4, 8] and step["stats"].tolist()[:2] == [12.0, 3.0]
    want = R.reseed_rows(step["best"].cpu().numpy(), 3)
    assert torch.equal(step["centres"][2:].cpu(), torch.from_numpy(f_h[want])) and set(want.tolist()) <= {2, 5, 8, 11}
    assert torch.allclose(step["centres"][:2].norm(dim=1).cpu(), torch.ones(2), atol=1e-5)


def test_pick_diverse():
    from spmm_amd import cluster as C
    f_h = R.pick_rows()
    f = _d(f_h)
    rr, rs, _ = R.farthest_first(f_h, 16, seed=R.PICK_SEED)
    rows, sim = C.pick_diverse(f, 16, seed=R.PICK_SEED)
    assert rows.dtype == torch.int64 and sim.dtype == torch.float32 and rows.tolist() == rr.tolist()
    assert sim[0].item() == float("-inf") and np.abs(sim.cpu().numpy()[1:] - rs[1:]).max() <= R.DELTA[64]
    again = C.pick_diverse(f, 16, seed=R.PICK_SEED)
    assert torch.equal(again[0], rows) and torch.equal(again[1].view(torch.int32), sim.view(torch.int32))
    assert C.pick_diverse(f, 3, first=77)[0].tolist() == R.farthest_first(f_h, 3, first=77)[0].tolist()
    assert C.pick_diverse(f, 2, seed=9)[0][0].item() == R.first_row(500, None, 9)
    dup = _d(np.concatenate([f_h[:6], f_h[:6], f_h[:6]]))
    picks = C.pick_diverse(dup, 6, first=8)[0]
    assert sorted((picks % 6).tolist()) == list(range(6)), "a copy was picked while another row remained"
    nan = f_h[:40].copy()
    nan[5] = np.nan
    assert 5 not in C.pick_diverse(_d(nan), 39, first=0)[0].tolist()
    index = type("Index", (), {"feats": f})()                     # anything with .feats, as a MoleculeIndex
    assert C.pick_diverse(index, 16, seed=R.PICK_SEED)[0].tolist() == rr.tolist()


def _rows(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


def test_driver_through_the_model(tmp_path):
    sys.path.insert(0, ROOT)
    import cluster
    base = ["--synthetic", "300", "--tiny", "--seed", "1"]
    out, meds, idx = tmp_path / "c.csv", tmp_path / "m.csv", tmp_path / "lib.idx"
    cluster.main(cluster.parse_args(base + ["--k", "5", "--output", str(out), "--medoids", str(meds), "--save_index", str(idx)]))
    rows = _rows(out)
    assert rows[0] == cluster.CLUSTER_HEADER and len(rows) == 301
    assert [int(r[0]) for r in rows[1:]] == list(range(1, 301)) and all(r[1] for r in rows[1:])
    clusters = [int(r[2]) for r in rows[1:]]
    assert set(clusters) <= set(range(5)) and all(-1.0 - 1e-5 <= float(r[3]) <= 1.0 + 1e-5 for r in rows[1:])
    medoids = [r for r in rows[1:] if r[4] == "1"]
    assert sorted(int(r[2]) for r in medoids) == sorted(set(clusters)), "one medoid per non-empty cluster"
    m = _rows(meds)
    assert m[0] == cluster.MEDOID_HEADER and len(m) == 6 and sum(int(r[1]) for r in m[1:]) == 300
    for r in m[1:]:
        assert int(r[1]) == clusters.count(int(r[0])) and (r[2] == "") == (int(r[1]) == 0)
        if r[2]:
            assert rows[int(r[2])][2] == r[0] and rows[int(r[2])][4] == "1" and rows[int(r[2])][1] == r[3]
    out2 = tmp_path / "c2.csv"
    cluster.main(cluster.parse_args(["--index", str(idx), "--k", "5", "--seed", "1", "--output", str(out2)]))
    assert _rows(out2) == rows, "--save_index then --index gives another CSV"
    picks = tmp_path / "p.csv"
    cluster.main(cluster.parse_args(base + ["--pick", "10", "--output", str(picks)]))
    p = _rows(picks)
    assert p[0] == cluster.PICK_HEADER and [int(r[0]) for r in p[1:]] == list(range(1, 11))
    assert len({r[1] for r in p[1:]}) == 10 and all(1 <= int(r[1]) <= 300 and r[2] for r in p[1:])
    assert p[1][3] == "" and all(-1.0 - 1e-5 <= float(r[3]) <= 1.0 + 1e-5 for r in p[2:])
    assert all(rows[int(r[1])][1] == r[2] for r in p[1:])
