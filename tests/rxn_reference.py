"""TEST INFRASTRUCTURE (never imported by spmm_amd/): reaction prediction as the reference runs it, restated sequentially -- one reaction at
a time, the whole prefix of every beam re-run at every position, host bookkeeping -- on the functional CPU oracle (oracle/spmm_oracle.py:
`bert_model` / `mlm_head`, which take a prefix and a BertCfg).

  encoder   `text_encoder2.bert.` : BertModel without cross-attention, mode='text' (layers 0 .. fusion_layer - 1)
  decoder   `text_encoder.`       : causal BertForMaskedLM, cross-attention to the encoded reactants under their mask
  evaluate        greedy: argmax per position for up to 100 positions, cut at the first [SEP]
  evaluate_beam   k x k candidates per position, [SEP] candidates recorded in row-major order and struck out with -1e5, the search ends once
                  k*k hypotheses are recorded; the k best after a stable descending sort

`RxnModule` exposes the same model through the module API (`text_encoder2.bert`, `text_encoder`, `generate`) so that code written against
that API (spmm_amd.decode.predict_products(cached=False)) runs on the oracle."""
from __future__ import annotations

import math
from dataclasses import replace
from types import SimpleNamespace
from typing import List, Tuple

import torch

import spmm_oracle as O

CLS_ID, SEP_ID = 2, 3
DEC, ENC = "text_encoder.", "text_encoder2."


def encoder_cfg(c_dec: O.BertCfg) -> O.BertCfg:
    return replace(c_dec, num_hidden_layers=c_dec.fusion_layer)


def rxn_keys(c_dec: O.BertCfg, c_enc: O.BertCfg):
    """(name, shape, kind) of the reaction model's state dict: decoder then encoder, each a BertForMaskedLM."""
    return (O._bert_keys(DEC + "bert.", c_dec, True) + O._mlm_keys(DEC, c_dec) + O._bert_keys(ENC + "bert.", c_enc, False) + O._mlm_keys(ENC, c_enc))


def closed_form_state_dict(c_dec: O.BertCfg, c_enc: O.BertCfg, scale: float = 0.08):
    """The oracle's closed-form initialiser (entry k, flat element i -> scale * sin(0.37 i + k); LayerNorm weights 1 + that) over both prefixes."""
    sd = {}
    for k, (name, shape, kind) in enumerate(rxn_keys(c_dec, c_enc)):
        n = int(math.prod(shape)) if shape else 1
        w = (scale * torch.sin(0.37 * torch.arange(n, dtype=torch.float64) + k)).to(torch.float32).reshape(shape)
        if kind == "posid":
            w = torch.arange(shape[1]).expand(1, -1).clone()
        elif kind == "ln_w":
            w = 1.0 + w
        sd[name] = w
    for p in (DEC, ENC):
        sd[p + "cls.predictions.decoder.weight"] = sd[p + "bert.embeddings.word_embeddings.weight"]
        sd[p + "cls.predictions.decoder.bias"] = sd[p + "cls.predictions.bias"]
    return sd


def random_state_dict(c_dec: O.BertCfg, c_enc: O.BertCfg, seed: int = 1, std: float = 0.08):
    """Seeded full-rank weights: N(0, std^2) matrices and embeddings, LayerNorm weights 1 + N(0, 0.05^2), biases N(0, 0.02^2).  The closed-form
    initialiser's matrices sin(0.37 i + k) have rank 2: whatever the decoder reads from its memory is squeezed through them and its next-token
    log-probabilities move by ~0.02 between reactions -- the searches return the same hypotheses for every reaction.  With these weights the
    hypotheses depend on the reactants (asserted where they are used)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape, kind in rxn_keys(c_dec, c_enc):
        if kind == "posid":
            w = torch.arange(shape[1]).expand(1, -1).clone()
        elif kind in ("emb", "lin_w"):
            w = torch.randn(shape, generator=g) * std
        elif kind == "ln_w":
            w = 1 + torch.randn(shape, generator=g) * 0.05
        else:
            w = torch.randn(shape, generator=g) * 0.02
        sd[name] = w
    for p in (DEC, ENC):
        sd[p + "cls.predictions.decoder.weight"] = sd[p + "bert.embeddings.word_embeddings.weight"]
        sd[p + "cls.predictions.decoder.bias"] = sd[p + "cls.predictions.bias"]
    return sd


def reaction(c: int, lens=(1, 3, 7, 16, 17, 24)) -> torch.Tensor:
    """Candidate reaction c: lens[c % len(lens)] reactant tokens from its own generator (seed 1000 + c)."""
    return torch.randint(4, 300, (lens[c % len(lens)],), generator=torch.Generator().manual_seed(1000 + c))


def pad_reactions(cands):
    rows = [reaction(c) for c in cands]
    ids = torch.zeros(len(rows), max(len(r) for r in rows), dtype=torch.long)
    for n, r in enumerate(rows):
        ids[n, :len(r)] = r
    return ids, (ids != 0).long()


def leaders_lm_bias(V: int, seed: int, k: int, margin: float, sep_margin: float, scale: float = 0.3) -> torch.Tensor:
    """N(0, scale^2) entries; the k - 1 largest are lifted by `margin` and [SEP] is set `sep_margin` >= margin above the k-th largest of the
    other tokens: the bias's k-th and (k+1)-th entries are at least `margin` apart, and which of the leaders a beam prefers is left to the
    hidden state."""
    assert sep_margin >= margin
    b = torch.randn(V, generator=torch.Generator().manual_seed(seed)) * scale
    b[SEP_ID] = -float("inf")
    top = torch.topk(b, k)
    b[top.indices[:k - 1]] += margin
    b[SEP_ID] = top.values[k - 1] + sep_margin
    return b


def lm_bias(V: int, seed: int, sep_gap: float) -> torch.Tensor:
    """A decoder LM bias that separates the next-token distributions and makes [SEP] a frequent runner-up: N(0, 1.5^2) entries, [SEP]'s set
    `sep_gap` below the largest."""
    b = torch.randn(V, generator=torch.Generator().manual_seed(seed)) * 1.5
    b[SEP_ID] = b.max() - sep_gap
    return b


def ranked_lm_bias(V: int, seed: int, k: int, margin: float, scale: float = 3.0) -> torch.Tensor:
    """N(0, scale^2) entries with [SEP]'s placed `margin` above the k-th largest of the other tokens.  With scale 3 on the closed-form model
    [SEP] is then the k-th largest: every beam offers it among its k candidates, decided by the bias and not by a near-tie (the hidden states of
    the tiny closed-form model move a logit by ~0.4 at most)."""
    b = torch.randn(V, generator=torch.Generator().manual_seed(seed)) * scale
    b[SEP_ID] = -float("inf")
    top = torch.topk(b, k).values
    b[SEP_ID] = top[k - 1] + margin
    return b


def with_lm_bias(sd, seed: int = 5, sep_gap: float = 1.5, bias: torch.Tensor | None = None):
    sd = dict(sd)
    b = lm_bias(sd[DEC + "cls.predictions.bias"].shape[0], seed, sep_gap) if bias is None else bias
    sd[DEC + "cls.predictions.bias"] = b
    sd[DEC + "cls.predictions.decoder.bias"] = b
    return sd


# ------------------------------------------------------------------------------------------------------------------ the model
@torch.no_grad()
def encode(sd, c_enc, ids: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    return O.bert_model(sd, ENC + "bert.", c_enc, False, input_ids=ids, attention_mask=mask, mode="text")


@torch.no_grad()
def decoder_logits(sd, c_dec, embeds: torch.Tensor, mask: torch.Tensor, prefix: torch.Tensor) -> torch.Tensor:
    """Logits [n, t, V] of the causal decoder on `prefix` [n, t] (0 = PAD) with cross-attention to embeds [1 or n, Lt, H] under mask."""
    n = prefix.shape[0]
    h = O.bert_model(sd, DEC + "bert.", c_dec, True, input_ids=prefix, attention_mask=(prefix != 0).long(), enc=embeds.expand(n, -1, -1),
                     enc_mask=mask.expand(n, -1), is_decoder=True)
    return O.mlm_head(sd, DEC, c_dec, h)


def _topk(last: torch.Tensor, k: int):
    top = torch.topk(torch.softmax(last.float(), dim=-1), k=k, dim=-1)
    return torch.log(top.values), top.indices


class RxnModule:
    """The reference's module API over the functional oracle, CPU fp32."""

    def __init__(self, sd, c_dec: O.BertCfg, c_enc: O.BertCfg):
        self.sd, self.c_dec, self.c_enc = sd, c_dec, c_enc
        self.text_encoder2 = SimpleNamespace(bert=self._encoder)

    def _encoder(self, input_ids, attention_mask=None, return_dict=True, mode="text"):
        assert mode == "text"
        return SimpleNamespace(last_hidden_state=encode(self.sd, self.c_enc, input_ids, attention_mask))

    def text_encoder(self, input_ids, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None, return_dict=True,
                     is_decoder=False, return_logits=False):
        assert is_decoder and return_logits
        return decoder_logits(self.sd, self.c_dec, encoder_hidden_states, encoder_attention_mask, input_ids)

    def generate(self, text_embeds, text_mask, product_input, stochastic=False, k=None):
        last = self.text_encoder(product_input, encoder_hidden_states=text_embeds, encoder_attention_mask=text_mask, is_decoder=True,
                                 return_logits=True)[:, -1, :]
        if k:
            return _topk(last, k)
        assert not stochastic
        return torch.argmax(last, dim=-1).unsqueeze(1)


def _cut(ids: torch.Tensor, mask: torch.Tensor):
    """One reaction's reactant tokens without their padding: ([1, L], [1, L])."""
    ids, mask = ids.reshape(-1), mask.reshape(-1)
    L = max(int(mask.sum()), 1)
    return ids[None, :L], mask[None, :L]


# ------------------------------------------------------------------------------------------------------------------ the searches
class SequentialBook:
    """The bookkeeping of `evaluate_beam` for one reaction, position by position, on the host."""

    def __init__(self, k: int, need: int | None = None):
        self.k, self.need = k, k * k if need is None else need
        self.finals: List[Tuple[float, List[int]]] = []
        self.stopped = False

    def first(self, values: torch.Tensor, indices: torch.Tensor):
        """values / indices [k]: the k best successors of [CLS]."""
        self.beams = [[CLS_ID, int(t)] for t in indices.tolist()]
        self.score = values.clone().float()

    def update(self, values: torch.Tensor, indices: torch.Tensor) -> bool:
        """values / indices [k, k]: per beam its k best next tokens.  Returns True once the search has stopped."""
        k = self.k
        cand_p = self.score[:, None] + values.float()
        found = False
        for b in range(k):
            for j in range(k):
                if int(indices[b, j]) == SEP_ID:
                    self.finals.append((float(cand_p[b, j]), self.beams[b] + [SEP_ID]))
                    cand_p[b, j] = -1e5
                    found = True
        if found and len(self.finals) >= self.need:
            self.stopped = True
            return True
        self.score, flat = torch.topk(cand_p.reshape(-1), k)
        self.beams = [self.beams[int(f) // k] + [int(indices[int(f) // k, int(f) % k])] for f in flat.tolist()]
        return False

    def results(self):
        return sorted(self.finals, key=lambda h: h[0], reverse=True)[:self.k]            # (sorted is stable)


@torch.no_grad()
def evaluate_beam(sd, c_dec, c_enc, ids: torch.Tensor, mask: torch.Tensor, k: int, max_steps: int = 100, need: int | None = None):
    """One reaction (ids / mask: its reactant tokens, padding allowed) -> up to k (log-prob, ids incl. [CLS] and [SEP]), best first.
    need: finals that end the search (None: k*k, the reference; k: the PV -> SMILES rule, for comparison)."""
    ids, mask = _cut(ids, mask)
    embeds = encode(sd, c_enc, ids, mask)
    book = SequentialBook(k, need)
    v, i = _topk(decoder_logits(sd, c_dec, embeds, mask, torch.tensor([[CLS_ID]]))[:, -1], k)
    book.first(v[0], i[0])
    for _ in range(max_steps):
        v, i = _topk(decoder_logits(sd, c_dec, embeds, mask, torch.tensor(book.beams))[:, -1], k)
        if book.update(v, i):
            break
    return book.results()


def evaluate(next_token, max_steps: int = 100) -> List[int]:
    """Greedy search of ONE reaction: next_token(prefix [1, t]) -> the most probable next id.  Returns the ids from [CLS] up to and including
    the first [SEP], or all max_steps + 1 of them."""
    seq = [CLS_ID]
    for _ in range(max_steps):
        seq.append(int(next_token(torch.tensor([seq]))))
        if seq[-1] == SEP_ID:
            break
    return seq


@torch.no_grad()
def evaluate_oracle(sd, c_dec, c_enc, ids, mask, max_steps: int = 100) -> List[int]:
    ids, mask = _cut(ids, mask)
    embeds = encode(sd, c_enc, ids, mask)
    return evaluate(lambda prefix: torch.argmax(decoder_logits(sd, c_dec, embeds, mask, prefix)[0, -1]), max_steps)


@torch.no_grad()
def evaluate_module(model, ids, mask, max_steps: int = 100) -> List[int]:
    """`evaluate` through a model's own module API (`text_encoder2.bert`, `generate`): the HIP model's facade loop, one reaction at a time."""
    ids, mask = _cut(ids, mask)
    embeds = model.text_encoder2.bert(ids, attention_mask=mask, return_dict=True, mode="text").last_hidden_state
    return evaluate(lambda prefix: model.generate(embeds, mask.to(embeds.device), prefix.to(embeds.device), stochastic=False)[0, 0], max_steps)


@torch.no_grad()
def score(sd, c_dec, c_enc, ids, mask, seq: List[int]) -> torch.Tensor:
    """Teacher-forced log-probabilities [len(seq) - 1] of the tokens seq[1:] under the oracle."""
    ids, mask = _cut(ids, mask)
    text = torch.tensor([seq])
    logits = decoder_logits(sd, c_dec, encode(sd, c_enc, ids, mask), mask, text)
    return torch.log_softmax(logits[0, :-1].float(), -1).gather(1, text[0, 1:, None])[:, 0]
