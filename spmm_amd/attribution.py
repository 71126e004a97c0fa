"""Cross-attention maps: which SMILES tokens each property attends to, and which properties each token attends to -- the head-averaged
(or per-head) attention probabilities of the fusion layers, the quantity the SPMM paper reads the learnt chemistry from; for the reaction
model, product-token -> reactant-token attention of the teacher-forced pass (the raw material of attention-based atom mapping).

The passes are the engine's own: every distinct molecule encoded once on packed rows, every distinct PV once, keys | values projected
once per distinct source and layer (retrieve.match_scores' batch; score._decode_scores' pass for reactions).  The probabilities come from
Engine.stack_fwd's `xattn_tap` -- views of the projected queries and keys both forms of the cross-attention block read -- and ONE
spmm_attn_probs launch (csrc/attnmap.hip) per tapped (layer, direction): fp32, nothing rounded to bf16, no [nseq, nH, Lq, Lkv] tensor
unless heads='all' asks for it.  Maps are an eval-mode quantity: no dropout."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .engine import BF, Batch, Group, KVSource, host_lens, host_token_count
from .score import _decode_scores, _engine, _inputs, _rxn_memory, check_pairs

TP = "text_encoder.bert."
DIRECTIONS = ("pv2text", "text2pv")
RXN_DIRECTION = "product2reactant"


@dataclass
class AttentionMaps:
    """Per pair, layer and direction an fp32 tensor [Lq_valid, Lkv_valid] (heads='mean') or [nH, Lq_valid, Lkv_valid] (heads='all'), padding
    cut off.  'pv2text': rows = [CLS] + the properties, columns = the molecule's tokens; 'text2pv': the transpose roles;
    'product2reactant': rows = product tokens, columns = reactant tokens.  `layers` are indices among the fusion layers, ascending."""
    pairs: torch.Tensor                 # int64 [P, 2] on the host
    layers: Tuple[int, ...]
    directions: Tuple[str, ...]
    heads: str
    maps: Dict[Tuple[int, int, str], torch.Tensor] = field(default_factory=dict)

    def get(self, pair: int, layer: int = -1, direction: Optional[str] = None) -> torch.Tensor:
        """pair: index into `pairs`; layer: an index among the fusion layers as it was requested (negative counts from the last
        requested); direction: may be left out when only one was requested."""
        if direction is None:
            if len(self.directions) != 1:
                raise ValueError(f"AttentionMaps.get: name one direction of {self.directions}")
            direction = self.directions[0]
        if direction not in self.directions:
            raise KeyError(f"AttentionMaps.get: direction {direction!r} was not requested (held: {self.directions})")
        if not 0 <= pair < self.pairs.shape[0]:
            raise IndexError(f"AttentionMaps.get: pair {pair} of {self.pairs.shape[0]}")
        if layer not in self.layers:
            if layer < 0 and -layer <= len(self.layers):
                layer = self.layers[layer]
            else:
                raise KeyError(f"AttentionMaps.get: layer {layer} was not requested (held: {self.layers})")
        return self.maps[(pair, layer, direction)]


def resolve_layers(layers, n_fusion: int, what: str) -> Tuple[int, ...]:
    """'all' or indices among the n_fusion fusion layers (negative from the last) -> ascending distinct indices in [0, n_fusion)."""
    if isinstance(layers, str):
        if layers != "all":
            raise ValueError(f"{what}: layers={layers!r} (indices among the {n_fusion} fusion layers, or 'all')")
        return tuple(range(n_fusion))
    if isinstance(layers, (int, np.integer)):
        layers = (layers,)
    out = set()
    for l in layers:
        if isinstance(l, bool) or not isinstance(l, (int, np.integer)) or not -n_fusion <= l < n_fusion:
            raise ValueError(f"{what}: unknown layer {l!r} (indices among the {n_fusion} fusion layers, or 'all')")
        out.add(int(l) % n_fusion)
    if not out:
        raise ValueError(f"{what}: no layer requested")
    return tuple(sorted(out))


def _check_modes(heads, direction, what):
    if heads not in ("mean", "all"):
        raise ValueError(f"{what}: heads={heads!r} (one of 'mean', 'all')")
    if direction not in DIRECTIONS + ("both",):
        raise ValueError(f"{what}: direction={direction!r} (one of 'pv2text', 'text2pv', 'both')")
    return DIRECTIONS if direction == "both" else (direction,)


class _Tap:
    """Engine.stack_fwd's xattn_tap: one spmm_attn_probs launch per wanted (layer, group); keeps [rows, Lkv] (and / or [nH, rows, Lkv])."""

    def __init__(self, nH: int, first_layer: int, layers, groups_wanted, heads: str):
        self.nH, self.first, self.layers, self.wanted, self.heads = nH, first_layer, set(layers), set(groups_wanted), heads
        self.out: Dict[Tuple[int, int], torch.Tensor] = {}
        self.qk: Dict[Tuple[int, int], tuple] = {}          # (tests, tools) the tapped views themselves, when keep_qk is set
        self.keep_qk = False

    def __call__(self, layer, gi, g, Q, K):
        li = layer - self.first
        if li not in self.layers or gi not in self.wanted:
            return
        if self.keep_qk:
            self.qk[(li, gi)] = (g, Q, K)
        all_heads = self.heads == "all"
        pm, ph = ops.attn_probs(Q, K, nseq=g.nseq, nH=self.nH, Lq=g.L, Lkv=g.Lkv, mean=not all_heads, heads=all_heads, **g.cross_layout())
        self.out[(li, gi)] = ph if all_heads else pm


def _cut(P_, row0: int, nq: int, nk: int) -> torch.Tensor:
    return P_[:, row0:row0 + nq, :nk] if P_.dim() == 3 else P_[row0:row0 + nq, :nk]      # (views of the launch's output: no copy per pair)


@torch.no_grad()
def cross_attention_maps(model, pv: torch.Tensor, prop_mask: Optional[torch.Tensor], ids: torch.Tensor, mask: torch.Tensor,
                         pairs: Optional[torch.Tensor] = None, *, layers=(-1,), heads: str = "mean", direction: str = "both",
                         _tap_hook=None) -> AttentionMaps:
    """Cross-attention maps of P (PV, molecule) pairs.  pv [Q, n_props] (normalised values); prop_mask (None, [n_props] or [Q, n_props],
    1 = property unknown: the learned mask token stands there); ids / mask [N, L]: token ids with '[CLS]' at position 0 and their
    attention masks (non-empty prefixes); pairs int64 [P, 2] = (row of pv, row of ids), None: row i with row i.
    layers: indices among the fusion layers (-1 the last) or 'all'; heads: 'mean' | 'all'; direction: 'pv2text' | 'text2pv' | 'both'
    (a direction that is not requested costs no launch).  All fusion layers run on all rows of the batch
    [P PV-query sequences, dense | P text-query sequences, packed], as retrieve.match_scores builds it.
    Raises ValueError for a molecule longer than ops.ATTN_MAXL tokens, a mask that is not a non-empty prefix, an unknown layer, head mode
    or direction; IndexError for a pair out of range."""
    from .decode import encode_properties
    what = "cross_attention_maps"
    dirs = _check_modes(heads, direction, what)
    ids_h, mask_h, lens_all = _inputs(ids, mask, what)
    pv = pv.reshape(-1, pv.shape[-1])
    pairs_h = check_pairs(pairs, pv.shape[0], ids_h.shape[0], what)
    eng = _engine(model)
    cfg, dev = model.cfg, eng.dev
    ct = cfg.text
    H, nH, Lp, f, n = ct.hidden_size, ct.num_attention_heads, cfg.n_props + 1, ct.fusion_layer, ct.num_hidden_layers
    lays = resolve_layers(layers, n - f, what)
    out = AttentionMaps(pairs_h, lays, dirs, heads)
    P = pairs_h.shape[0]
    if P == 0:
        return out
    if prop_mask is not None:
        prop_mask = prop_mask.reshape(-1, pv.shape[1]).expand(pv.shape[0], pv.shape[1])
    qs, inv_q = torch.unique(pairs_h[:, 0], return_inverse=True)
    ms, inv_m = torch.unique(pairs_h[:, 1], return_inverse=True)
    Up = qs.numel()
    # ---- every distinct molecule's text, once, on packed rows (cut to the longest of them)
    lens_u = lens_all[ms.numpy()]
    Lt = int(lens_u.max())
    if Lt > ops.ATTN_MAXL:
        raise ValueError(f"{what}: a molecule of {Lt} tokens exceeds the {ops.ATTN_MAXL} the packed attention layouts hold")
    mask_u = mask_h[ms, :Lt]
    t = eng.encode_text(TP, ct, ids_h[ms, :Lt].to(dev).to(torch.int32).contiguous(), mask_u.to(dev).to(torch.int32).contiguous(),
                        n_tokens=host_token_count(mask_u))
    # ---- every distinct PV, once
    pv_d = pv.to(dev).to(torch.float32)[qs.to(dev)]
    pe = encode_properties(model, pv_d, None if prop_mask is None else prop_mask.to(dev)[qs.to(dev)])        # [Up, Lp, H]
    eng.train_mode = False
    pvh = pe.to(BF).reshape(Up * Lp, H).contiguous()
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)                        # noqa: E731
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)                        # noqa: E731
    src_text = t.source(tables=True)
    src_pv = KVSource(pvh, Up, Lp)
    # ---- the fusion batch: [P PV-query sequences, dense | P text-query sequences, packed]; every fusion layer on every row
    iq, im = inv_q.numpy(), inv_m.numpy()
    len_p, qrow0, Mt, _, _, gat_tx = t.pair_layout(lens_u, im)
    o_t = P * Lp
    gat_pv = (iq[:, None] * Lp + np.arange(Lp)[None, :]).reshape(-1)
    X = torch.cat([pvh.index_select(0, i64(gat_pv)), t.y.index_select(0, i64(gat_tx))])
    batch = Batch([Group(0, P, Lp, None, P).bind(src_text, i32(im), 0),
                   Group(o_t, P, Lt, None, P, q_row0=i32(qrow0), q_len=i32(len_p), nrows=Mt).bind(src_pv, i32(iq), 0)])
    gidx = {"pv2text": 0, "text2pv": 1}
    tap = _Tap(nH, f, lays, [gidx[d] for d in dirs], heads)
    if _tap_hook is not None:
        _tap_hook(tap)
    eng.stack_fwd(TP, ct, range(f, n), True, X, batch, False, xattn_tap=tap)
    for li in lays:
        for d in dirs:
            P_ = tap.out[(li, gidx[d])]
            for p in range(P):
                if d == "pv2text":
                    out.maps[(p, li, d)] = _cut(P_, p * Lp, Lp, int(len_p[p]))
                else:
                    out.maps[(p, li, d)] = _cut(P_, int(qrow0[p]), int(len_p[p]), Lp)
    return out


@torch.no_grad()
def reaction_attention_maps(model, src_ids: torch.Tensor, src_mask: torch.Tensor, prod_ids: torch.Tensor, prod_mask: torch.Tensor,
                            pairs: Optional[torch.Tensor] = None, *, layers=(-1,), heads: str = "mean", _tap_hook=None) -> AttentionMaps:
    """Product-token -> reactant-token attention of P (reactants, product) pairs on the reaction model (spmm_amd.rxn.SPMMRxn): the
    teacher-forced pass of score.score_products, tapped.  Arguments as score_products; per pair and requested decoder layer (indices among
    the layers that cross-attend, -1 the last, or 'all') a map [product tokens, reactant tokens] (direction 'product2reactant').
    Errors as cross_attention_maps; a product of one token ('[CLS]' alone) has no pass to tap and is refused."""
    what = "reaction_attention_maps"
    if heads not in ("mean", "all"):
        raise ValueError(f"{what}: heads={heads!r} (one of 'mean', 'all')")
    sids_h, smask_h, slens = _inputs(src_ids, src_mask, what + " (sources)")
    pids_h, pmask_h, plens = _inputs(prod_ids, prod_mask, what + " (products)")
    pairs_h = check_pairs(pairs, sids_h.shape[0], pids_h.shape[0], what)
    eng = _engine(model)
    ct = model.cfg.text
    f, n = ct.fusion_layer, ct.num_hidden_layers
    lays = resolve_layers(layers, n - f, what)
    out = AttentionMaps(pairs_h, lays, (RXN_DIRECTION,), heads)
    P = pairs_h.shape[0]
    if P == 0:
        return out
    len_p = plens[pairs_h[:, 1].numpy()]
    if int(len_p.max()) < 2:
        raise ValueError(f"{what}: every product is '[CLS]' alone: there is no decoder pass to read")
    src, inv_s = _rxn_memory(model, eng, sids_h, slens, pairs_h, what)
    tap = _Tap(ct.num_attention_heads, f, lays, [0], heads)
    if _tap_hook is not None:
        _tap_hook(tap)
    _decode_scores(eng, ct, pids_h, plens, torch.stack([inv_s, pairs_h[:, 1]], dim=1), src, True, pids_h.shape[1], what, xattn_tap=tap)
    len_s = slens[pairs_h[:, 0].numpy()]
    qrow0 = np.concatenate([[0], np.cumsum(len_p)[:-1]])
    for li in lays:
        P_ = tap.out[(li, 0)]
        for p in range(P):
            out.maps[(p, li, RXN_DIRECTION)] = _cut(P_, int(qrow0[p]), int(len_p[p]), int(len_s[p]))
    return out
