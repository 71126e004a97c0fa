"""TEST INFRASTRUCTURE (not collected): the sequential one-molecule PV -> SMILES beam search of oracle/decode_oracle.py::beam_search, started
from a given prefix instead of [CLS] alone -- the yard-stick of the prompted searches of spmm_amd.decode.  Built on the imported
`decode_oracle.next_token_topk` (one whole-prefix forward per position) with that search's bookkeeping order: the k successors of the
prefix, then per position the k x k candidates, [SEP] candidates recorded in row-major order and struck out with -1e5, stop at k finals,
the k best survive.  Scores count the generated tokens only."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

import decode_oracle                                            # oracle/ (tests/conftest.py puts it on the path)

SEP_ID = decode_oracle.SEP_ID


def peaky_lm(sd, seed: int = 5, sep_gap: float = 1.5):
    """The decode tests' LM-head bias (`_peaky_lm`): N(0, 1.5^2) entries, [SEP]'s `sep_gap` below the largest, under both tied keys."""
    b = torch.randn(sd["text_encoder.cls.predictions.bias"].shape, generator=torch.Generator().manual_seed(seed)) * 1.5
    b[SEP_ID] = b.max() - sep_gap
    sd = dict(sd)
    sd["text_encoder.cls.predictions.bias"] = b
    sd["text_encoder.cls.predictions.decoder.bias"] = b
    return sd


def prefixes(N: int, P: int, seed: int, V: int = 300) -> torch.Tensor:
    """[N, P] token ids: [CLS], then P - 1 seeded non-special tokens per molecule."""
    p = torch.randint(4, V, (N, P), generator=torch.Generator().manual_seed(seed))
    p[:, 0] = decode_oracle.CLS_ID
    return p


@torch.no_grad()
def beam_search_with_prefix(model, prop: torch.Tensor, prefix: Sequence[int], k: int = 5, max_steps: int = 100) -> List[Tuple[float, List[int]]]:
    """One molecule (prop [53]) from `prefix` ([CLS] p1 ..) -> up to k finished hypotheses (log-prob of the generated tokens, ids with the
    prefix and [SEP]), best first.  max_steps counts positions after the first generated token, as in `beam_search`."""
    from spmm_amd.decode import encode_properties
    pv = encode_properties(model, prop.reshape(1, -1))
    start = torch.tensor([list(prefix)], dtype=torch.long, device=pv.device)
    lp, tok = decode_oracle.next_token_topk(model, pv, start, k)
    beams = torch.cat([start.expand(k, -1), tok.reshape(k, 1)], dim=1)
    beam_lp = lp.reshape(k)
    finals: List[Tuple[float, torch.Tensor]] = []
    for _ in range(max_steps):
        lp, tok = decode_oracle.next_token_topk(model, pv, beams, k)
        cand_lp = beam_lp[:, None] + lp
        cand = torch.cat([beams[:, None, :].expand(k, k, -1), tok[:, :, None]], dim=2)
        for b, j in (tok == SEP_ID).nonzero(as_tuple=False).tolist():
            finals.append((float(cand_lp[b, j]), cand[b, j].clone()))
            cand_lp[b, j] = -1e5
        if len(finals) >= k:
            break
        beam_lp, keep = torch.topk(cand_lp.reshape(-1), k)
        beams = cand.reshape(k * k, -1)[keep]
    finals.sort(key=lambda h: h[0], reverse=True)
    return [(p, ids.tolist()) for p, ids in finals[:k]]
