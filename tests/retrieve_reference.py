"""TEST INFRASTRUCTURE (never imported by spmm_amd/): the retrieval quantities as the reference computes them, restated in fp32 on the CPU
over the functional oracle (oracle/spmm_oracle.py: `bert_model`, `_lin` and the state dict's head weights), one pair at a time and every
molecule at its own length -- no padding, no packing, no sharing of anything between pairs.

  pv_hidden / pv_features       SPMM_models.py:82-92 without the MPM draw; prop_mask = 1 puts `property_mask` at an unknown property
  text_hidden / smiles_features SPMM_models.py:93-95
  match_prob                    SPMM_models.py:137-152, 199-202: softmax(itm_head(cat(cls_p, cls_t)))[:, 1]

`RetrieveModule` is the oracle's module view with the three heads added, so that code written against the module API
(spmm_amd.retrieve.match_scores(engine=False)) runs on the oracle."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import spmm_oracle as O

TP = "text_encoder.bert."


def pv_hidden(sd, cfg, pv: torch.Tensor, prop_mask=None) -> torch.Tensor:
    """[Q, n_props] -> the PV encoder's hidden states [Q, n_props + 1, H]."""
    Q = pv.shape[0]
    feat = F.linear(pv.unsqueeze(2), sd["property_embed.weight"], sd["property_embed.bias"])
    if prop_mask is not None:
        mk = prop_mask.to(feat.dtype).reshape(-1, pv.shape[1]).expand(Q, -1).unsqueeze(2)
        feat = feat * (1 - mk) + sd["property_mask"].expand(Q, feat.shape[1], -1) * mk
    properties = torch.cat([sd["property_cls"].expand(Q, -1, -1), feat], dim=1)
    with torch.no_grad():
        return O.bert_model(sd, "property_encoder.", cfg.prop, False, inputs_embeds=properties)


def pv_features(sd, cfg, pv, prop_mask=None):
    h = pv_hidden(sd, cfg, pv, prop_mask)
    with torch.no_grad():
        return F.normalize(O._lin(sd, "property_proj", h[:, 0, :], f32_out=True), dim=-1), h


def text_hidden(sd, cfg, ids_row: torch.Tensor) -> torch.Tensor:
    """One molecule at its own length: ids_row [L] without padding -> [1, L, H]."""
    with torch.no_grad():
        return O.bert_model(sd, TP, cfg.text, True, input_ids=ids_row[None, :], attention_mask=torch.ones(1, ids_row.numel(), dtype=torch.long),
                            mode="text")


def _rows(ids, mask):
    return [ids[b, :int(mask[b].sum())] for b in range(ids.shape[0])]


def smiles_features(sd, cfg, ids, mask) -> torch.Tensor:
    with torch.no_grad():
        cls = torch.cat([text_hidden(sd, cfg, r)[:, 0, :] for r in _rows(ids, mask)])
        return F.normalize(O._lin(sd, "text_proj", cls, f32_out=True), dim=-1)


def itm_logits(sd, cls_p, cls_t):
    return O._lin(sd, "itm_head", torch.cat([cls_p, cls_t], dim=-1), f32_out=True, f32_w=True)


def match_prob(sd, cfg, pv_h: torch.Tensor, ids, mask, pairs) -> torch.Tensor:
    """pv_h [Q, Lp, H] fp32 (pv_hidden's output); pairs [P, 2] = (query, molecule) -> [P]."""
    tc = cfg.text
    rows = _rows(ids, mask)
    out = []
    with torch.no_grad():
        for qi, mi in pairs.tolist():
            pv = pv_h[qi:qi + 1]
            text = text_hidden(sd, cfg, rows[mi])
            ones_p = torch.ones(pv.shape[:2], dtype=torch.long)
            ones_t = torch.ones(text.shape[:2], dtype=torch.long)
            cls_p = O.bert_model(sd, TP, tc, True, encoder_embeds=pv, attention_mask=ones_p, enc=text, enc_mask=ones_t, mode="fusion")[:, 0, :]
            cls_t = O.bert_model(sd, TP, tc, True, encoder_embeds=text, attention_mask=ones_t, enc=pv, enc_mask=ones_p, mode="fusion")[:, 0, :]
            out.append(torch.softmax(itm_logits(sd, cls_p, cls_t), dim=-1)[0, 1])
    return torch.stack(out)


class RetrieveModule(O.OracleModule):
    """OracleModule + the heads retrieval calls as modules."""

    def itm_head(self, x):
        return O._lin(self.sd, "itm_head", x, f32_out=True, f32_w=True)

    def property_proj(self, x):
        return O._lin(self.sd, "property_proj", x, f32_out=True)

    def text_proj(self, x):
        return O._lin(self.sd, "text_proj", x, f32_out=True)


def spread_itm_head(sd, scale: float):
    """The closed-form itm_head weight times `scale` (a copy of the state dict): its two rows are nearly parallel sinusoids, so the two
    logits move together and the matching probability barely moves between pairs; a larger weight spreads them."""
    sd = dict(sd)
    sd["itm_head.weight"] = sd["itm_head.weight"] * scale
    return sd


# ------------------------------------------------------------------------------------------------------------------ the shared case
LT = 24
PAIRS = [(0, 0), (0, 2), (0, 4), (1, 2), (2, 2), (1, 1), (2, 3)]      # query 0 meets three molecules, molecule 2 three queries; molecule 0 has 2 tokens


def path_case():
    """5 molecules of 2, 3, 20, LT - 1 and LT tokens ([CLS] first, [SEP] last), 3 property vectors, the third with 20 properties unknown."""
    g = torch.Generator().manual_seed(31)
    lens = [2, 3, 20, LT - 1, LT]
    ids = torch.zeros(len(lens), LT, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, 0] = 2
        if n > 2:
            ids[b, 1:n - 1] = torch.randint(4, 300, (n - 2,), generator=g)
        ids[b, n - 1] = 3
    mask = (ids != 0).long()
    pv = torch.randn(3, 53, generator=g)
    prop_mask = torch.zeros(3, 53)
    prop_mask[2, torch.randperm(53, generator=g)[:20]] = 1
    return ids, mask, pv, prop_mask, torch.tensor(PAIRS, dtype=torch.long)


def library_case(n: int = 40, seed: int = 9):
    """n molecules of n DISTINCT token counts 3 .. n + 2 in a seeded random order: whatever order the rows are given in, sorting them by
    length gives the same sequence, so length-sorted batches hold the same molecules in the same places."""
    g = torch.Generator().manual_seed(seed)
    lens = (torch.randperm(n, generator=g) + 3).tolist()
    L = n + 2
    ids = torch.zeros(n, L, dtype=torch.long)
    for b, ln in enumerate(lens):
        ids[b, 0] = 2
        ids[b, 1:ln - 1] = torch.randint(4, 300, (ln - 2,), generator=g)
        ids[b, ln - 1] = 3
    pv = torch.randn(3, 53, generator=g)
    prop_mask = torch.zeros(3, 53)
    prop_mask[1, ::3] = 1
    return ids, (ids != 0).long(), pv, prop_mask
