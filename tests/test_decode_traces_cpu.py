"""The launches of every decode search, pinned: with ops._DRY_RUN a tiny model on the CPU runs whole searches and ops._dry_log records every
launch by name.  What the docstrings of spmm_amd/decode.py promise "launch for launch" is what this file holds them to."""
import collections
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "decode_launch_traces.json")
PRE = [2, 10, 11, 12]                                   # [CLS] and three pieces: a prefix no grammar reads (the syntax variants start from [CLS])
KW = dict(k=2, max_steps=6, sync_every=64)              # sync_every > max_steps: no host decision reads what a dry launch left unwritten


def _traces():
    """{variant: the names of its launches, in order}."""
    from spmm_amd import decode as D, ops
    from spmm_amd import smiles_syntax as SS
    from spmm_amd.config import tiny_config
    from spmm_amd.model import SPMM
    from spmm_amd.rxn import SPMMRxn
    old, old_fused = ops._DRY_RUN, D.FUSED_BEAM_STEP
    ops._DRY_RUN = True
    try:
        m = SPMM(spmm_config=tiny_config(), no_train=True, device="cpu").eval()
        rxn = SPMMRxn(bert_config=tiny_config().text, device="cpu")
        vocab = [str(x) for x in np.load(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz"), allow_pickle=False)["vocab"]]
        table = SS.SyntaxTable.from_vocab(vocab)
        props = torch.randn(6, 53, generator=torch.Generator().manual_seed(1))
        ids = torch.randint(4, 300, (3, 9), generator=torch.Generator().manual_seed(2))
        mask = torch.ones(3, 9, dtype=torch.long)
        mask[1, 4:] = 0
        beam = lambda **kw: D.beam_search_batched(m, props, **KW, **kw)                                             # noqa: E731
        distinct = lambda **kw: D.sample_distinct(m, props[:2], 12, seed=3, max_steps=6, sync_every=64, **kw)      # noqa: E731

        def tensor_ops():
            D.FUSED_BEAM_STEP = False
            try:
                return beam(stochastic=True, seed=3)
            finally:
                D.FUSED_BEAM_STEP = old_fused

        variants = {
            "beam": beam,
            "seeded": lambda: beam(stochastic=True, seed=3),
            "prefix_prefill": lambda: beam(prefix=PRE, prefill=True),
            "prefix_steps": lambda: beam(prefix=PRE, prefill=False),
            "temperature": lambda: beam(temperature=0.8),
            "guided_top_p": lambda: beam(guidance=2.0, top_p=0.9),
            "guided_prefix": lambda: beam(guidance=2.0, prefix=PRE),
            "generate_chunked_guided": lambda: D.generate_with_property(m, props[0], 5, k=2, seed=3, max_steps=6, chunk=2, guidance=2.0),
            "distinct": distinct,
            "distinct_top_p": lambda: distinct(top_p=0.9),
            "distinct_prefix": lambda: distinct(prefix=PRE),
            "seeded_tensor_ops": tensor_ops,
            "syntax": lambda: beam(syntax=table),
            "syntax_guided": lambda: beam(syntax=table, guidance=2.0),
            "syntax_distinct": lambda: distinct(syntax=table),
            "predict_products": lambda: D.predict_products(rxn, ids, mask, **KW),
        }
        out = {}
        for name, run in variants.items():
            ops._dry_log.clear()
            run()
            out[name] = list(ops._dry_log)
        return out
    finally:
        ops._DRY_RUN = old
        ops._dry_log.clear()


def _summary(log):
    return dict(launches=len(log), sha256=hashlib.sha256("\n".join(log).encode()).hexdigest(), counts=dict(sorted(collections.Counter(log).items())))


def test_every_search_issues_the_recorded_launches():
    """Plain, seeded, prefixed (prefill and stepped), warped, guided, chunked generation, distinct, the tensor-op bookkeeping, the three
    constrained searches and reaction prediction, tiny configuration, 6 property vectors, k = 2, 6 positions: per variant the launch count
    per kernel and the SHA-256 of the whole name sequence equal tests/golden/decode_launch_traces.json.
    The fixture is a record of the code BEFORE a change that must not alter the launches.  Re-record it only when a change is meant to
    alter them, at the commit the change starts from or with the change reviewed launch by launch:
        python tests/test_decode_traces_cpu.py --record"""
    with open(FIXTURE) as f:
        want = json.load(f)
    got = {name: _summary(log) for name, log in _traces().items()}
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name]["counts"] == want[name]["counts"], name
        assert got[name]["launches"] == want[name]["launches"] and got[name]["sha256"] == want[name]["sha256"], name


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(pytest.main([__file__, *sys.argv[1:]]))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    with open(FIXTURE, "w") as f:
        json.dump({name: _summary(log) for name, log in _traces().items()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {FIXTURE}")
