"""cluster.py --threshold / --dedup: parsing, the refusals before any model is built, and the CSVs of a stubbed run (the tensor-library form
of spmm_amd.cluster.leaders on CPU features stands in for the engine; no GPU, no model run)."""
import csv
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cluster  # noqa: E402

import butina_reference as B  # noqa: E402

BASE = ["--synthetic", "300", "--tiny"]


def test_flags_parse():
    a = cluster.parse_args(BASE + ["--threshold", "0.8", "--order", "row", "--max_pairs", "1000", "--medoids", "m.csv"])
    assert (a.threshold, a.order, a.max_pairs, a.dedup, a.k, a.pick, a.medoids) == (0.8, "row", 1000, None, 0, 0, "m.csv")
    b = cluster.parse_args(BASE + ["--dedup", "0.98"])
    assert (b.dedup, b.threshold, b.order, b.max_pairs) == (0.98, None, "count", 1 << 30)
    c = cluster.parse_args(BASE + ["--k", "5"])
    assert c.threshold is None and c.dedup is None, "without the flags the run is the k-means one"
    with pytest.raises(SystemExit):
        cluster.parse_args(BASE + ["--threshold", "0.8", "--order", "size"])


@pytest.mark.parametrize("argv, msg", [
    (["--threshold", "0.8", "--k", "5"], "--threshold and --k are alternatives"),
    (["--threshold", "0.8", "--pick", "5"], "--k, --pick, --threshold and --dedup are alternatives"),
    (["--threshold", "0.8", "--dedup", "0.9"], "--k, --pick, --threshold and --dedup are alternatives"),
    (["--dedup", "0.9", "--k", "5"], "--k, --pick, --threshold and --dedup are alternatives"),
    (["--threshold", "1.5"], r"--threshold 1.5 is not a cosine in \[-1, 1\]"),
    (["--threshold", "nan"], "--threshold nan is not a cosine"),
    (["--dedup", "-3"], r"--dedup -3.0 is not a cosine in \[-1, 1\]"),
    (["--threshold", "0.5", "--max_pairs", "-1"], "--max_pairs must be at least 0"),
    (["--dedup", "0.9", "--medoids", "m.csv"], "--medoids goes with --k or --threshold"),
])
def test_main_refuses_before_a_model_is_built(argv, msg, monkeypatch):
    import spmm_amd.model as model_mod
    monkeypatch.setattr(model_mod, "SPMM", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a model was built")))
    with pytest.raises(SystemExit, match=msg):
        cluster.main(cluster.parse_args(BASE + ["--device", "cpu"] + argv))


def test_threshold_alone_gets_as_far_as_the_device_check():
    with pytest.raises(SystemExit, match="--device cpu: spmm_amd has no CPU / eager fallback"):
        cluster.main(cluster.parse_args(BASE + ["--threshold", "0.8", "--device", "cpu"]))
    with pytest.raises(SystemExit, match="--device cpu: spmm_amd has no CPU / eager fallback"):
        cluster.main(cluster.parse_args(BASE + ["--dedup", "0.8", "--medoids", "", "--device", "cpu"]))


class _Index:
    def __init__(self, feats, smiles):
        self.feats, self.smiles = feats, smiles

    def __len__(self):
        return self.feats.shape[0]


def _stub():
    from spmm_amd import cluster as C
    return types.SimpleNamespace(leaders=lambda index, t, order, max_pairs: C.leaders(index, t, order=order, max_pairs=max_pairs, engine=False))


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_threshold_csvs_on_a_stubbed_run(tmp_path, capsys):
    f, label = B.planted_groups()
    N = len(label)
    index = _Index(torch.from_numpy(f), [f"C{i}" for i in range(N)])
    out, meds = tmp_path / "c.csv", tmp_path / "m.csv"
    args = cluster.parse_args(BASE + ["--threshold", str(B.MIX_THRESHOLD), "--output", str(out), "--medoids", str(meds)])
    cluster.main_leaders(args, index, _stub())
    rows = _read(out)
    assert rows[0] == ["library_line", "smiles", "cluster", "cosine_to_centre", "is_medoid", "n_neighbours"] and len(rows) == N + 1
    assert [int(r[0]) for r in rows[1:]] == list(range(1, N + 1)) and rows[1][1] == "C0"
    sizes = sorted(B.GROUP_SIZES, reverse=True)
    for r in rows[1:]:
        assert sizes[int(r[2])] == B.GROUP_SIZES[label[int(r[0]) - 1]] and int(r[5]) == sizes[int(r[2])] - 1
        assert (r[4] == "1") == (float(r[3]) == 1.0) and float(r[3]) >= B.MIX_THRESHOLD
    assert sum(r[4] == "1" for r in rows[1:]) == len(sizes)
    m = _read(meds)
    assert m[0] == cluster.MEDOID_HEADER and [int(r[1]) for r in m[1:]] == sizes
    for r in m[1:]:
        assert rows[int(r[2])][2] == r[0] and rows[int(r[2])][4] == "1" and rows[int(r[2])][1] == r[3]
    text = capsys.readouterr().out
    assert "12 clusters (order count), 0 singletons" in text and "cluster sizes: min 5, median 47, max 120" in text
    assert f"{sum(s * (s - 1) for s in sizes) // 2} pairs at or above" in text and "rounds" in text and "max degree 119" in text
    assert text.count("leader line") == 10


def test_dedup_csv_on_a_stubbed_run(tmp_path, capsys):
    f, first = B.dedup_library()
    N = len(first)
    index = _Index(torch.from_numpy(f), [f"C{i}" for i in range(N)])
    out = tmp_path / "u.csv"
    args = cluster.parse_args(BASE + ["--dedup", str(B.DEDUP_THRESHOLD), "--output", str(out)])
    cluster.main_leaders(args, index, _stub())
    rows = _read(out)
    kept = np.nonzero(first == np.arange(N))[0]
    assert rows[0] == ["library_line", "smiles"] and [int(r[0]) for r in rows[1:]] == (kept + 1).tolist()
    assert all(r[1] == f"C{int(r[0]) - 1}" for r in rows[1:])
    text = capsys.readouterr().out
    assert f"{N - len(kept)} of {N} lines dropped" in text
    for i in np.nonzero(first != np.arange(N))[0]:
        assert "line %-8d dropped: a duplicate of line %d" % (i + 1, first[i] + 1) in text


def test_too_many_pairs_ends_the_run_with_the_flag_named(tmp_path):
    f, _ = B.planted_groups()
    index = _Index(torch.from_numpy(f), None)
    args = cluster.parse_args(BASE + ["--threshold", "0.6", "--max_pairs", "10", "--output", str(tmp_path / "c.csv")])
    with pytest.raises(SystemExit, match=r"neighbour entries at threshold .* exceed max_pairs=10 \(--max_pairs\)"):
        cluster.main_leaders(args, index, _stub())
    assert not (tmp_path / "c.csv").exists()
