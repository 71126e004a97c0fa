"""cluster.py: what the driver decides from its arguments alone -- parsing, the refusals before any model is built -- and its CSV writers
on hand-made results (no GPU, no model run)."""
import csv
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cluster  # noqa: E402

BASE = ["--synthetic", "300", "--tiny"]


def test_flags_parse():
    a = cluster.parse_args(BASE + ["--k", "5", "--iters", "7", "--init", "random", "--seed", "1", "--medoids", "m.csv", "--output", "o.csv"])
    assert (a.k, a.iters, a.init, a.seed, a.medoids, a.output, a.pick, a.synthetic, a.tiny) == (5, 7, "random", 1, "m.csv", "o.csv", 0, 300, True)
    b = cluster.parse_args(["--index", "lib.idx", "--pick", "10", "--save_index", "x.idx", "--batch_size", "64", "--host_tokenizer"])
    assert (b.pick, b.k, b.index, b.save_index, b.batch_size, b.init, b.iters) == (10, 0, "lib.idx", "x.idx", 64, "farthest", 20)
    assert b.host_tokenizer and b.device == "cuda" and b.checkpoint and b.vocab_filename
    with pytest.raises(SystemExit):
        cluster.parse_args(BASE + ["--k", "5", "--init", "nearest"])
    assert cluster.MAX_K == 65536
    from spmm_amd import cluster as C
    assert C.MAX_K == cluster.MAX_K


@pytest.mark.parametrize("argv, msg", [
    (["--k", "5", "--pick", "3"], "--k and --pick are alternatives"),
    ([], r"give --k K \(cluster the library\) or --pick N"),
    (["--k", "301"], r"--k 301 outside \[1, 300\]"),
    (["--k", "-2"], r"--k -2 outside \[1, 65536\]"),
    (["--k", "65537"], r"--k 65537 outside \[1, 65536\]"),
    (["--pick", "301"], r"--pick 301 outside \[1, 300\]"),
    (["--pick", "-1"], "--pick -1 must be at least 1"),
    (["--k", "5", "--iters", "0"], "--iters must be at least 1"),
    (["--pick", "5", "--medoids", "m.csv"], "--medoids goes with --k"),
    (["--k", "5", "--library", "x.txt", "--index", "y.idx"], "--library and --index are alternatives"),
])
def test_main_refuses_before_a_model_is_built(argv, msg, monkeypatch):
    import spmm_amd.model as model_mod
    monkeypatch.setattr(model_mod, "SPMM", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a model was built")))
    synth = [] if "--library" in argv else BASE
    with pytest.raises(SystemExit, match=msg):
        cluster.main(cluster.parse_args(synth + ["--device", "cpu"] + argv))


def test_the_library_is_needed_and_its_size_bounds_k(tmp_path, monkeypatch):
    import spmm_amd.model as model_mod
    monkeypatch.setattr(model_mod, "SPMM", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a model was built")))
    with pytest.raises(SystemExit, match="give the library"):
        cluster.main(cluster.parse_args(["--k", "3", "--device", "cpu"]))
    lib = tmp_path / "lib.txt"
    lib.write_text("CCO\nCCN\nc1ccccc1\n")
    with pytest.raises(SystemExit, match=r"--k 4 outside \[1, 3\] \(the library has 3 molecules\)"):
        cluster.main(cluster.parse_args(["--library", str(lib), "--k", "4", "--device", "cpu"]))
    with pytest.raises(SystemExit, match=r"--pick 9 outside \[1, 3\]"):
        cluster.main(cluster.parse_args(["--library", str(lib), "--pick", "9", "--device", "cpu"]))


def test_a_device_without_a_gpu_is_refused_with_a_clear_message():
    with pytest.raises(SystemExit, match="--device cpu: spmm_amd has no CPU / eager fallback"):
        cluster.main(cluster.parse_args(BASE + ["--k", "5", "--device", "cpu"]))


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_cluster_csv(tmp_path):
    smiles = ["CCO", "CCN", "c1ccccc1", "C,C"]                                     # (a comma: the writer quotes it)
    assign = torch.tensor([1, 0, 1, 1], dtype=torch.int32)
    best = torch.tensor([0.5, 1.0, 0.25, 0.75])
    medoid = torch.tensor([1, 3, -1], dtype=torch.int32)
    rows = cluster.cluster_rows(assign, best, medoid, smiles)
    assert rows == [(1, "CCO", 1, "0.5", 0), (2, "CCN", 0, "1.0", 1), (3, "c1ccccc1", 1, "0.25", 0), (4, "C,C", 1, "0.75", 1)]
    out = tmp_path / "c.csv"
    cluster.write_csv(str(out), cluster.CLUSTER_HEADER, rows)
    got = _read(out)
    assert got[0] == ["library_line", "smiles", "cluster", "cosine_to_centre", "is_medoid"]
    assert got[4] == ["4", "C,C", "1", "0.75", "1"] and len(got) == 5
    assert cluster.cluster_rows(assign, best, medoid, None)[0][1] == ""
    meds = cluster.medoid_rows(torch.tensor([1, 3, 0]), medoid, smiles)
    assert meds == [(0, 1, 2, "CCN"), (1, 3, 4, "C,C"), (2, 0, "", "")]
    cluster.write_csv(str(out), cluster.MEDOID_HEADER, meds)
    got = _read(out)
    assert got[0] == ["cluster", "size", "library_line", "smiles"] and got[3] == ["2", "0", "", ""]
    assert cluster.size_summary(torch.tensor([5, 1, 9, 3])) == (1, 5, 9)


def test_pick_csv(tmp_path):
    smiles = ["CCO", "CCN", "c1ccccc1"]
    rows = cluster.pick_rows(torch.tensor([2, 0]), torch.tensor([float("-inf"), 0.125]), smiles)
    assert rows == [(1, 3, "c1ccccc1", ""), (2, 1, "CCO", "0.125")]
    out = tmp_path / "p.csv"
    cluster.write_csv(str(out), cluster.PICK_HEADER, rows)
    got = _read(out)
    assert got[0] == ["pick_order", "library_line", "smiles", "max_cosine_to_earlier_picks"] and got[1] == ["1", "3", "c1ccccc1", ""]
