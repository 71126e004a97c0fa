"""TEST INFRASTRUCTURE (never imported by spmm_amd/): the reaction model's training loss, `SPMM_rxn.forward` (SPMM_models_rxn.py:31-46), on the
functional CPU oracle with autograd enabled (rxn_reference.decoder_logits runs under no_grad and cannot serve a gradient check), plus the
batches and weight sets the training tests share."""
from __future__ import annotations

import torch

import spmm_oracle as O
import rxn_reference as R

SRC_LENS, SRC_L = (1, 3, 7, 16, 17, 24, 9, 24), 24
PROD_LENS, PROD_L = (1, 2, 5, 12, 20, 8, 3, 20), 20         # 71 valid tokens, 63 labels; sequence 0 has none, sequences 4 and 7 end at L - 1


def sequences(lens, L, seed, vocab=300):
    """[CLS] tokens [SEP] PAD... of the given lengths -> (ids int64 [n, L], mask)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), L, dtype=torch.long)
    for i, n in enumerate(lens):
        ids[i, 0] = R.CLS_ID
        if n > 2:
            ids[i, 1:n - 1] = torch.randint(4, vocab, (n - 2,), generator=g)
        if n > 1:
            ids[i, n - 1] = R.SEP_ID
    return ids, (ids != 0).long()


def batch(seed=0, src_lens=SRC_LENS, prod_lens=PROD_LENS, src_L=SRC_L, prod_L=PROD_L):
    """-> (src_ids, src_mask, prod_ids, prod_mask)"""
    return sequences(src_lens, src_L, 10 + seed) + sequences(prod_lens, prod_L, 20 + seed)


def labels(prod_ids: torch.Tensor) -> torch.Tensor:
    """int64 [B, L - 1]: the target of position t is token t + 1; 0 = ignored."""
    return prod_ids[:, 1:].clone()


def ce_ignore0(logits: torch.Tensor, prod_ids: torch.Tensor) -> torch.Tensor:
    """(1/n) sum over the n positions with a non-PAD target of -log softmax(logits[b, t])[ids[b, t + 1]]; logits [B, L, V]."""
    lab = labels(prod_ids)
    keep = lab != 0
    lp = torch.log_softmax(logits[:, :-1], dim=-1).gather(2, lab[..., None])[..., 0]
    return (-(lp * keep).sum()) / keep.sum()


def logits(sd, c_dec, c_enc, src_ids, src_mask, prod_ids, prod_mask, train=False):
    emb = O.bert_model(sd, R.ENC + "bert.", c_enc, False, input_ids=src_ids, attention_mask=src_mask, mode="text", train=train)
    h = O.bert_model(sd, R.DEC + "bert.", c_dec, True, input_ids=prod_ids, attention_mask=prod_mask, enc=emb, enc_mask=src_mask, is_decoder=True,
                     train=train)
    return O.mlm_head(sd, R.DEC, c_dec, h)


def loss(sd, c_dec, c_enc, src_ids, src_mask, prod_ids, prod_mask, train=False) -> torch.Tensor:
    return ce_ignore0(logits(sd, c_dec, c_enc, src_ids, src_mask, prod_ids, prod_mask, train), prod_ids)


def leaves(sd, c_dec, c_enc):
    """The state dict as autograd leaves (aliases re-tied) -> (sd, names of the parameters)."""
    sd = {k: v.clone() for k, v in sd.items()}
    names = [n for n, _, k in R.rxn_keys(c_dec, c_enc) if k not in ("posid", "tied_w", "tied_b")]
    for n in names:
        sd[n].requires_grad_(True)
    for p in (R.DEC, R.ENC):
        sd[p + "cls.predictions.decoder.weight"] = sd[p + "bert.embeddings.word_embeddings.weight"]
        sd[p + "cls.predictions.decoder.bias"] = sd[p + "cls.predictions.bias"]
    return sd, names


UNTOUCHED = tuple(R.ENC + "cls.predictions." + s for s in ("bias", "transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight",
                                                           "transform.LayerNorm.bias", "decoder.bias"))
