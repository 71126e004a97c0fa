"""pv2smiles.py --distinct: what the driver decides from its arguments alone -- the refusals, the note about the ignored flags, the
--n_generate limit -- before any model is built (no GPU, no model run)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pv2smiles  # noqa: E402

BASE = ["--synthetic", "--tiny", "--distinct"]


def test_the_flag_parses_and_is_off_by_default():
    assert pv2smiles.parse_args(["--synthetic"]).distinct is False
    args = pv2smiles.parse_args(BASE + ["--n_generate", "64", "--seed", "1", "--syntax"])
    assert args.distinct is True and args.n_generate == 64 and args.syntax


def test_the_note_names_the_ignored_flags():
    lines = pv2smiles.distinct_args(pv2smiles.parse_args(BASE + ["--n_generate", "64", "--k", "5", "--chunk", "16"]))
    assert len(lines) == 1 and "--k 5" in lines[0] and "--chunk 16" in lines[0] and "ignored" in lines[0] and "64 slots" in lines[0]


@pytest.mark.parametrize("n", [1, 8, 1000, 1024])
def test_up_to_1024_samples_are_accepted(n):
    assert pv2smiles.distinct_args(pv2smiles.parse_args(BASE + ["--n_generate", str(n)]))
    from spmm_amd import decode
    assert pv2smiles.DISTINCT_MAX == decode.DISTINCT_MAX == 1024


@pytest.mark.parametrize("argv, msg", [
    (["--n_generate", "1025"], r"--n_generate 1025 outside \[1, 1024\]"),
    (["--n_generate", "5000"], r"at most 1024 distinct sequences"),
    (["--n_generate", "0"], r"--n_generate 0 outside \[1, 1024\]"),
    (["--guidance", "2"], r"--guidance 2 is not available with --distinct"),
    (["--guidance", "0"], r"--guidance 0 is not available with --distinct"),
    (["--stochastic", "False"], r"--stochastic False asks for the deterministic beam search"),
    (["--temperature", "0"], r"temperature=0.0 must be finite and > 0"),
    (["--top_p", "1.5"], r"top_p=1.5 outside \(0, 1\]"),
])
def test_main_refuses_before_a_model_is_built(argv, msg, monkeypatch):
    import spmm_amd.model as model_mod
    monkeypatch.setattr(model_mod, "SPMM", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a model was built")))
    with pytest.raises(SystemExit, match=msg):
        pv2smiles.main(pv2smiles.parse_args(BASE + ["--n_generate", "16", "--device", "cpu"] + argv))


def test_a_top_k_below_the_beams_of_a_decoder_row_is_fine_with_distinct():
    """Without --distinct every beam keeps --k tokens and a smaller --top_k is refused; the distinct search keeps 1."""
    from spmm_amd import decode
    assert decode.check_warp(1.0, 1.0, 1, 1.0, 1) == dict(guidance=1.0, temperature=1.0, top_k=1, top_p=1.0)
    with pytest.raises(ValueError, match="top_k=1 is below the k=2"):
        decode.check_warp(1.0, 1.0, 1, 1.0, 2)


def test_without_the_flag_the_refusals_do_not_apply():
    """--n_generate 5000, --guidance 2 and --stochastic False stay what they were: nothing of --distinct is consulted."""
    args = pv2smiles.parse_args(["--synthetic", "--n_generate", "5000", "--guidance", "2", "--stochastic", "False"])
    assert args.distinct is False and args.n_generate == 5000 and args.stochastic is False
