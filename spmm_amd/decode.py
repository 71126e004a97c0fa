"""PV -> SMILES k-beam decoding (BASELINE.json configs[3]): N molecules x k beams per launch with
a key/value cache, returning per molecule the hypotheses the reference's one-molecule, whole-prefix-per-step search
(`generate`, d_pv2smiles_single.py:26-51; `evaluate`, d_pv2smiles_batched.py:18-59) returns.  That sequential search is
restated in oracle/decode_oracle.py -- test infrastructure, the yard-stick of tests/ -- not here.
How the searches are put together: `make_decoder` builds the decoder of every search (K/V cache or whole-prefix forwards, with or without
a warp, one half or two); a decoder's `step` / `prefill` return logits that have gone their last mile (`_Decoder.finish`: grammar mask
on the raw logits, then the warp), so a search masks exactly once and never asks what class it drives; `_start` begins the beam
searches (`_search`, behind beam_search_batched, generate_with_property and predict_products) and the distinct one (sample_distinct)
alike; `_advance` is the one position of the former, `_GumbelNoise` the seeded noise of both."""
from __future__ import annotations

import functools
import math
import random
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops                # (reached as module attributes at call time: bench.py wraps ops.gemm_nt, ops.decode_attn, ops.ln_fwd)

CLS_ID, SEP_ID = 2, 3           # vocab_bpe_300.txt:3-4
GRAPH_BELOW_ROWS = 200          # measured break-even of graph=True, not a switch (replay is opt-in): with the bookkeeping in one launch a position is a
#                                 chain of ~130 dependent kernels (1.95 ms at 100 rows, 2.2 at 1 000, 3.6 at 5 000) and replay gains 7 % at 100 rows, 2 % at
#                                 250, nothing from 500 on -- and a replayed graph has a fixed batch: no compaction of finished molecules
last_run: dict = {}             # what the last eager _search did: molecules, compactions, final_batch, positions, prefix_tokens, prefill, the decoder's
#                                 warp_info (guidance, temperature, top_k, top_p, baseline_rows: 0, or the N*k rows of the all-masked half), syntax
#                                 (the decoder carried a mask), dropped_masked (finals a constrained search dropped: they went through a masked token)
COMPACT_BELOW = 0.75            # the batch is re-gathered once at most this share of its molecules is still live
FUSED_BEAM_STEP = True          # beam bookkeeping of a position as one HIP launch (spmm_beam_step); False: the tensor-op form (BeamBook.update)
GUMBEL_SALT = 0x50563253        # call-site salt of the sampled search's noise ("PV2S"; dropout and negative sampling use small integers)
last_generate: dict = {}        # what the last generate_with_property did: samples, no_final, chunks, prefix_tokens, the warp_info of the last chunk's
#                                 decoder (last_run's five), syntax (bool), dropped_masked (summed over the chunks)


def _pick(p: torch.Tensor, k: int, stochastic: bool, generator=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two k-candidate branches of `generate` (d_pv2smiles_single.py:37-44): the k most probable next tokens, or k
    tokens drawn without replacement from the next-token distribution.  p: [..., V] probabilities -> (log-probs, ids) [..., k]."""
    if stochastic:
        flat = p.reshape(-1, p.shape[-1])
        ids = torch.multinomial(flat, num_samples=k, replacement=False, generator=generator)
        return torch.log(flat.gather(1, ids)).reshape(*p.shape[:-1], k), ids.reshape(*p.shape[:-1], k)
    top = torch.topk(p, k=k, dim=-1)
    return torch.log(top.values), top.indices


# ------------------------------------------------------------------------------------------------------------------
# Seeded sampling: Gumbel noise from a counter.  Adding independent Gumbel(0, 1) noise to the logits and taking the k largest, in
# descending order, IS k draws without replacement from softmax(logits), in draw order (Gumbel-top-k) -- what torch.multinomial(p, k,
# replacement=False) does in the reference.  Every element hashes its own index (global molecule, position, beam, token), so a molecule's
# draws do not depend on the batch it is decoded in.  Device form: csrc/decode.hip::gumbel_noise_kernel; this is the same arithmetic on
# the host (integers identical, the transform in float64).
# ------------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def gumbel_bits_host(seed: int, salt: int, mol_ids, t: int, k: int, V: int, Lmax: int) -> np.ndarray:
    """The 24-bit integers x = rng_pair(seed_mix(seed, salt), idx) >> 8 of csrc/common.h for idx = ((mol * Lmax + t) * k + b) * V + j:
    int64 [len(mol_ids), k, V].  mol_ids are GLOBAL molecule indices (mol_base + n)."""
    key = _splitmix64((_splitmix64(int(seed) & _M64) + int(salt)) & _M64)
    mol = np.asarray(mol_ids, dtype=np.uint64).reshape(-1, 1, 1)
    b = np.arange(k, dtype=np.uint64).reshape(1, k, 1)
    j = np.arange(V, dtype=np.uint64).reshape(1, 1, V)
    with np.errstate(over="ignore"):
        idx = ((mol * np.uint64(Lmax) + np.uint64(t)) * np.uint64(k) + b) * np.uint64(V) + j
        lo, hi = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
        x = (lo ^ np.uint32(key & 0xFFFFFFFF)) + (hi ^ np.uint32(key >> 32)) * np.uint32(0x9E3779B1)
        x ^= x >> np.uint32(16); x *= np.uint32(0x21F0AAAD)
        x ^= x >> np.uint32(15); x *= np.uint32(0x735A2D97)
        x ^= x >> np.uint32(15)
    return (x >> np.uint32(8)).astype(np.int64)


def gumbel_noise_host(seed: int, salt: int, mol_ids, t: int, k: int, V: int, Lmax: int) -> torch.Tensor:
    """Gumbel noise of ops.gumbel_noise on the host: float64 [len(mol_ids) * k, V], g = -log(-log(u)), u = (x + 0.5) * 2^-24 in (0, 1)."""
    u = (gumbel_bits_host(seed, salt, mol_ids, t, k, V, Lmax).astype(np.float64) + 0.5) * 2.0 ** -24
    return torch.from_numpy(-np.log(-np.log(u))).reshape(-1, V)


class _GumbelNoise:
    """The noise of one seeded search, beam or distinct: `noise(t, mol)` -> [n * k, V] for the position t of the last token held, for the
    molecules now in the batch (mol: BeamBook.mol, None = all).  ids (host int64 [N]): the GLOBAL molecule every molecule of the batch
    draws as -- mol_base + n for the beam searches, (pv_base + g) * 128 + slot // 8 for the distinct one.  On the device (fp32, one
    buffer) where spmm_gumbel_noise takes the shape (k <= 8, V <= 512, Lmax <= 256: whatever the one-launch steps take), else the host
    form in float64 -- which only ever serves the whole batch."""

    def __init__(self, seed: int, salt: int, ids: torch.Tensor, k: int, V: int, Lmax: int, device, on_device: bool):
        self.seed, self.salt, self.ids, self.shape, self.device = seed, salt, ids, (k, V, Lmax), device
        self.buf = torch.empty(ids.numel() * k, V, dtype=torch.float32, device=device) if on_device else None
        if on_device:
            self.seed_dev = torch.tensor([(int(seed) & _M64) - ((int(seed) & (1 << 63)) << 1)], dtype=torch.int64, device=device)
            self.ids_dev = ids.to(torch.int32).to(device)
            self.mol = self.live = None                  # the last compaction seen and the ids of its molecules

    def __call__(self, t: int, mol: torch.Tensor | None = None) -> torch.Tensor:
        k, V, Lmax = self.shape
        if self.buf is None:
            return gumbel_noise_host(self.seed, self.salt, self.ids.tolist(), t, k, V, Lmax).to(self.device)
        if mol is not None and mol is not self.mol:      # (gathered once per compaction, not per position)
            self.mol, self.live = mol, self.ids_dev[mol.long()]
        ids = self.ids_dev if mol is None else self.live
        return ops.gumbel_noise(self.seed_dev, ids.numel(), k, V, Lmax, salt=self.salt, t=t, mol=ids, out=self.buf[:ids.numel() * k])


def _pick_seeded(logits: torch.Tensor, noise: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The sampled branch of `_pick` with explicit noise, on LOGITS [..., V]: ids = the k largest of logits + noise in descending order,
    log-probs = log_softmax(logits) at those ids (unperturbed) -> (log-probs, ids) [..., k].  The tensor-op twin of the SAMPLED
    instantiation of csrc/decode.hip::beam_step_kernel: both form the keys with the same single fp32 add."""
    ids = torch.topk(logits + noise.to(logits.dtype).reshape(logits.shape), k=k, dim=-1).indices
    return torch.log_softmax(logits, dim=-1).gather(-1, ids), ids


# ------------------------------------------------------------------------------------------------------------------
# The distribution the search draws from: guidance towards the condition, temperature, top-k and nucleus truncation.
# ------------------------------------------------------------------------------------------------------------------
def check_warp(guidance: float, temperature: float, top_k: int, top_p: float, k: int) -> dict | None:
    """The four sampling controls of the searches -> None when all are at their defaults (the search is then today's, launch for launch),
    else dict(guidance, temperature, top_k, top_p).  ValueError for temperature <= 0 or not finite, top_p outside (0, 1], top_k < 0 or not
    an integer, a non-finite guidance, and an explicit top_k in [1, k): every beam draws k distinct tokens, so k are always kept
    (min_keep) and a smaller request would be overridden silently."""
    if isinstance(top_k, bool) or int(top_k) != top_k:
        raise ValueError(f"top_k={top_k!r} must be an integer >= 0 (0: no top-k cut)")
    guidance, temperature, top_k, top_p = float(guidance), float(temperature), int(top_k), float(top_p)
    if not math.isfinite(guidance):
        raise ValueError(f"guidance={guidance} must be finite (1: the conditioned model alone, 0: the all-masked baseline, > 1: towards the condition)")
    if not (math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"temperature={temperature} must be finite and > 0")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p={top_p} outside (0, 1]")
    if top_k < 0:
        raise ValueError(f"top_k={top_k} must be >= 0 (0: no top-k cut)")
    if 0 < top_k < k:
        raise ValueError(f"top_k={top_k} is below the k={k} tokens every beam draws: k tokens are always kept, ask for top_k >= k (or 0)")
    if guidance == 1.0 and temperature == 1.0 and top_k == 0 and top_p == 1.0:
        return None
    return dict(guidance=guidance, temperature=temperature, top_k=top_k, top_p=top_p)


NO_WARP = dict(guidance=1.0, temperature=1.0, top_k=0, top_p=1.0)


def warp_logits(lc: torch.Tensor, lu: torch.Tensor | None = None, *, guidance: float = 1.0, temperature: float = 1.0, top_k: int = 0,
                top_p: float = 1.0, min_keep: int = 1) -> torch.Tensor:
    """The rules of spmm_logit_warp (include/spmm_hip.h; csrc/warp.hip) as tensor ops, any device and dtype, over the last dimension:
      1. g = lu + guidance * (lc - lu), the classifier-free contrast between the conditioned logits lc and the all-masked ones lu (raw
         logits: the constants of the two log-softmaxes vanish in the next softmax); lu=None: g = lc;
      2. z = g / temperature (temperature == 1: z = g);
      3. tokens ranked by (z descending, index ascending);
      4. K = top_k if 0 < top_k < V else V, q = softmax of z over the K best; rank r is kept iff r < min_keep, or r < K and the q-mass of
         the ranks < r is < top_p (top_p == 1: no nucleus cut);
      5. z where kept, -inf elsewhere.
    The searches read the result as logits: the recorded log-probabilities are those of the warped distribution, renormalised over the
    kept tokens.  The route of every search the one-launch beam step does not take, and the float64 reference of the kernel's tests.
    With every argument at its default the input comes back as it is."""
    g = lc if lu is None else lu + guidance * (lc - lu)
    z = g if temperature == 1.0 else g / temperature
    V = z.shape[-1]
    K = int(top_k) if 0 < int(top_k) < V else V
    if K == V and top_p >= 1.0:
        return z
    zs, order = torch.sort(z, dim=-1, descending=True, stable=True)          # (stable: equal values keep their index order)
    r = torch.arange(V, device=z.device)
    e = torch.exp(zs - zs[..., :1]) * (r < K).to(zs.dtype)
    before = (torch.cumsum(e, dim=-1) - e) / e.sum(dim=-1, keepdim=True)
    keep_sorted = (r < min_keep) | ((r < K) & ((before < top_p) if top_p < 1.0 else torch.ones_like(before, dtype=torch.bool)))
    keep = torch.zeros_like(keep_sorted).scatter(-1, order, keep_sorted)
    return torch.where(keep, z, torch.full_like(z, -float("inf")))


# ------------------------------------------------------------------------------------------------------------------
# Syntax-constrained search: the grammar mask on the raw next-token logits (smiles_syntax.py: grammar, cost, invariant).
# ------------------------------------------------------------------------------------------------------------------
SYNTAX_DROP_BELOW = -1e29       # a final at or below this score went through a masked token (the mask writes -1e30): it is not returned


def syntax_table(model, syntax, prefix=None, max_steps: int | None = None):
    """The `syntax` argument of the searches -> None (None / False: the search of today) or a smiles_syntax.SyntaxTable (True: built from
    model.tokenizer's vocabulary, once per tokenizer).  ValueError when there is no tokenizer, when the vocabulary cannot pay the grammar's
    cost one token at a time, when the table is not the model's vocabulary, and -- with max_steps -- when a prefix (check_prefix's result;
    None: [CLS] alone) rejects or cannot be closed within max_steps tokens."""
    if syntax is None or syntax is False:
        return None
    from . import smiles_syntax as SS
    if syntax is True:
        tok = getattr(model, "tokenizer", None)
        if tok is None or not hasattr(tok, "itos"):
            raise ValueError("syntax=True builds the grammar table from model.tokenizer and this model has none: set model.tokenizer, or pass a "
                             "smiles_syntax.SyntaxTable")
        table = getattr(tok, "_syntax_table", None)
        if table is None or table.pieces != list(tok.itos):
            table = tok._syntax_table = SS.SyntaxTable.from_vocab(tok.itos)
    elif isinstance(syntax, SS.SyntaxTable):
        table = syntax
    else:
        raise ValueError(f"syntax={syntax!r}: None, a bool or a smiles_syntax.SyntaxTable")
    V = _vocab_size(model)
    if V is not None and V != table.V:
        raise ValueError(f"syntax: the table holds {table.V} pieces, the model's vocabulary {V}")
    if (table.cls_id, table.sep_id) != (CLS_ID, SEP_ID):
        raise ValueError(f"syntax: [CLS] / [SEP] at {table.cls_id} / {table.sep_id}, the search expects {CLS_ID} / {SEP_ID}")
    if max_steps is not None:
        rows = [[CLS_ID]] if prefix is None else sorted({tuple(r) for r in prefix.tolist()})
        for r in rows:
            SS.check_prefix_state(table, list(r), max_steps)
    return table


class SyntaxMask:
    """The grammar mask of one constrained search: `mask(lc, lu, by=...)` strikes (smiles_syntax.MASKED, in place) the next-token logits
    lc [rows, V] -- and lu, the guidance baseline, alike -- that cannot follow the rows' histories.  Before the book exists (`book` None)
    the histories are the prefixes: by="pair" rows are the (condition, prefix) pairs of a prefill, by="row" the N*k beam rows; afterwards
    they are the book's own token histories (through `book.mol` once the batch is compacted), kept current by the beam step.
    kernel=True: one launch (ops.smiles_mask); else smiles_syntax.allowed per row on the host -- slow and correct: whole-prefix decoders,
    the tensor-op bookkeeping, shapes the kernel does not take."""

    def __init__(self, table, k: int, P: int, max_steps: int, device, kernel: bool):
        self.table, self.k, self.P, self.t_last, self.Lmax = table, k, P, P + max_steps, P + max_steps + 2
        self.device, self.kernel, self.book = device, bool(kernel), None
        self.dev_table = torch.from_numpy(table.packed).to(device) if kernel else None
        self.pair_hist = self.row_hist = None

    def start(self, prefix: torch.Tensor | None, pom, N: int):
        """prefix: int64 [Npairs, P] on the host (None: [CLS] alone); pom [N]: the pair of every molecule."""
        if prefix is None:
            self.row_hist = torch.full((N * self.k, 1), CLS_ID, dtype=torch.int32)
        else:
            self.pair_hist = prefix.to(torch.int32).contiguous()
            self.row_hist = self.pair_hist[torch.as_tensor(pom).to(torch.int64)].repeat_interleave(self.k, dim=0).contiguous()
        if self.kernel:
            self.row_hist = self.row_hist.to(self.device)
            self.pair_hist = None if self.pair_hist is None else self.pair_hist.to(self.device)

    def __call__(self, lc: torch.Tensor, lu: torch.Tensor | None = None, by: str = "row"):
        if self.book is None:
            hist, t, k, mol = (self.pair_hist if by == "pair" else self.row_hist), self.P, 1, None
        else:
            hist, t, k, mol = self.book.tokens, self.book.t, self.k, self.book.mol
        if lc.shape[-1] != self.table.V:
            raise ValueError(f"syntax: the table holds {self.table.V} pieces, the logits {lc.shape[-1]}")
        if self.kernel:
            ops.smiles_mask(lc, hist, self.dev_table, t=t, t_last=self.t_last, k=k, mol=mol, Lmax=self.Lmax, logits2=lu)
            return
        from . import smiles_syntax as SS
        rows = hist.reshape(-1, hist.shape[-1])[:, :t].cpu().tolist()
        assert len(rows) == lc.shape[0] and mol is None, (len(rows), lc.shape)
        keep = torch.from_numpy(np.stack([SS.allowed(self.table, r, self.t_last) for r in rows])).to(lc.device)
        lc.masked_fill_(~keep, SS.MASKED)
        if lu is not None:
            lu.masked_fill_(~keep, SS.MASKED)


@torch.no_grad()
def encode_properties(model, prop: torch.Tensor, prop_mask: torch.Tensor | None = None) -> torch.Tensor:
    """d_pv2smiles_batched.py:24-27: PV [B,53] -> prop_embeds [B,54,H].  prop_mask ([53] or [B,53], 1 = property unknown)
    substitutes the learned mask token for those entries, as conditional generation on a subset of properties does
    (d_pv2smiles_single.py:66-70)."""
    feat = model.property_embed(prop.unsqueeze(2))
    if prop_mask is not None:
        mk = prop_mask.to(feat.device).to(feat.dtype).reshape(-1, prop.shape[1])[..., None]
        unk = model.property_mask.detach().to(feat.device).to(feat.dtype).expand(feat.shape[0], feat.shape[1], -1)
        feat = feat * (1 - mk) + unk * mk
    cls = model.property_cls
    properties = torch.cat([cls.expand(feat.size(0), -1, -1).to(feat.dtype).to(feat.device), feat], dim=1)
    return model.property_encoder(inputs_embeds=properties, return_dict=True).last_hidden_state


# ------------------------------------------------------------------------------------------------------------------
# Batched decoding: N molecules x k beams per launch, key/value cache, no host round trips inside the loop.
# ------------------------------------------------------------------------------------------------------------------
def _set_column(x: torch.Tensor, t, v):
    """x[..., t] = v for a column t on the host (int) or in device memory (int64 [1]: no host read); v: a scalar or a tensor of x's
    shape without the last dimension."""
    if isinstance(t, int):
        x[..., t] = v
    elif torch.is_tensor(v):
        x.index_copy_(-1, t, v.unsqueeze(-1))
    else:
        x.index_fill_(-1, t, v)


class BeamBook:
    """The beam bookkeeping of the reference's search for N independent molecules at once, as tensor ops (no `.item()`):
    per molecule it makes exactly the decisions d_pv2smiles_batched.py:29-57 makes -- candidates ending in [SEP] are moved to
    `final` in row-major order and struck out with -1e5, the molecule stops once it holds >= k finals, the k best of the
    k*k candidates survive.  need (None: k): the number of finals that stops a molecule -- `evaluate_beam` of reaction prediction
    (d_rxn_prediction.py:86-123) searches on until k*k hypotheses have ended; `results` returns the k best either way."""

    def __init__(self, N: int, k: int, max_steps: int, device, fused: bool = False, need: int | None = None, prefix: torch.Tensor | None = None):
        """prefix (int [N, P], P >= 1, prefix[:, 0] = [CLS]): every beam of molecule n starts from prefix[n] instead of [CLS] alone; the
        search then generates up to max_steps + 1 further tokens.  Scores count the generated tokens only, finals carry the prefix."""
        P = 1 if prefix is None else int(prefix.shape[1])
        self.P = P
        self.N, self.k, self.Lmax = N, k, P + max_steps + 2
        self.need = k if need is None else int(need)
        if not k <= self.need <= k * k:
            raise ValueError(f"need={need} outside [k, k*k] = [{k}, {k * k}]")
        self.F = self.need + k                            # < need finals before the last appending step, <= k appended by it (one [SEP] per beam)
        it = torch.int32 if fused else torch.long         # fused: the state csrc/decode.hip::beam_step_kernel updates in place
        self.fused = fused
        self.tokens = torch.zeros(N, k, self.Lmax, dtype=it, device=device)
        if prefix is None:
            self.tokens[:, :, 0] = CLS_ID
        else:
            self.tokens[:, :, :P] = prefix.to(device).to(it)[:, None, :]
        self.t = P                                        # tokens held by every live beam
        self.cur_p = torch.zeros(N, k, device=device)
        self.fin_p = torch.full((N, self.F + 1), -float("inf"), device=device)           # slot F is a write-only dump
        self.fin_len = torch.zeros(N, self.F + 1, dtype=it, device=device)
        self.fin_tok = torch.zeros(N, self.F + 1, self.Lmax, dtype=it, device=device)
        self.fin_n = torch.zeros(N, dtype=it, device=device)
        self.done = torch.zeros(N, dtype=torch.bool, device=device)
        self.n_done = torch.zeros(1, dtype=torch.int32, device=device) if fused else None
        self.mol = None                                   # fused, after compact(): int32 indices of the molecules still decoded

    def first(self, values: torch.Tensor, indices: torch.Tensor):
        """values/indices [N,k]: log-probs and ids of the k best successors of [CLS] (of the prefix: the token at position P)."""
        self.tokens[:, :, self.P] = indices
        self.cur_p = values.clone()
        self.t = self.P + 1

    def update(self, values: torch.Tensor, indices: torch.Tensor, t: torch.Tensor | None = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """values/indices [N,k,k]: per live beam the k best next tokens.  Returns (parent [N,k], token [N,k]) of the new beams.
        The number of tokens held by the live beams is self.t, advanced here -- or `t` (int64 [1]) in device memory, self.t then left to
        the caller: nothing of the call sequence depends on the position (graph replay).  The state is updated in place either way."""
        N, k, F, L = self.N, self.k, self.F, self.Lmax
        host = t is None
        if host:
            t = self.t
        k2_p = (self.cur_p[:, :, None] + values).reshape(N, k * k)
        idx = indices.reshape(N, k * k)
        ends = (idx == SEP_ID) & ~self.done[:, None]
        e = ends.long()
        slot = torch.where(ends, self.fin_n[:, None] + torch.cumsum(e, 1) - e, torch.full_like(e, F))
        self.fin_p.scatter_(1, slot, k2_p)
        self.fin_len.scatter_(1, slot, e * (t + 1))        # (0 for the candidates that go to the dump slot)
        cand = self.tokens[:, :, None, :].expand(N, k, k, L).reshape(N, k * k, L).clone()
        _set_column(cand, t, SEP_ID)
        self.fin_tok.scatter_(1, slot[:, :, None].expand(N, k * k, L), cand)
        self.fin_n += e.sum(1)
        k2_p = torch.where(ends, torch.full_like(k2_p, -1e5), k2_p)
        new_p, flat = torch.topk(k2_p, k, dim=1)
        parent = flat // k
        tok = idx.gather(1, flat)
        live = ~(self.done | (self.fin_n >= self.need))   # a molecule that just reached its finals breaks before this update
        new_tokens = self.tokens.gather(1, parent[:, :, None].expand(N, k, L))
        _set_column(new_tokens, t, tok)
        torch.where(live[:, None, None], new_tokens, self.tokens, out=self.tokens)
        torch.where(live[:, None], new_p, self.cur_p, out=self.cur_p)
        self.done |= self.fin_n >= self.need
        if host:
            self.t = t + 1
        return parent, tok

    def live_slots(self) -> torch.Tensor:
        """Positions (in the current, possibly compacted batch) of the molecules that are not done yet."""
        done = self.done if self.mol is None else self.done[self.mol.long()]
        return (~done).nonzero().squeeze(1)

    def compact(self, keep: torch.Tensor):
        """Keep only the batch slots `keep` (from live_slots()); the state arrays stay whole, the kernel indexes them through `mol`."""
        cur = torch.arange(self.N, dtype=torch.int32, device=self.done.device) if self.mol is None else self.mol
        self.mol = cur[keep].contiguous()

    def step_fused(self, logits: torch.Tensor, anc: torch.Tensor | None = None, t_ptr: torch.Tensor | None = None, t_off: int = 0,
                   ids_out: torch.Tensor | None = None, rowmap: torch.Tensor | None = None, noise: torch.Tensor | None = None) -> torch.Tensor:
        """`update` (and the decoder's ancestry reorder) as one HIP launch on the next-token logits [N*k, V]: softmax, the k best successors
        per beam, finals, survivors, token histories, `anc` -- all in place.  Returns the tokens to feed next (int32 [N*k]).  With t_ptr
        (device int32 [1]) the number of tokens held comes from device memory (*t_ptr + t_off) and self.t is left to the caller.  With noise
        (fp32 [N*k, V]) the k successors of a beam are the k largest of logits + noise: the sampled search."""
        ids = ops.beam_step(logits, self, t=self.t, t_ptr=t_ptr, t_off=t_off, anc=anc, ids_out=ids_out, rowmap=rowmap, noise=noise)
        if t_ptr is None:
            self.t += 1
        return ids

    def all_done(self) -> bool:
        """Host check (one small device read): every molecule holds its finals."""
        return int(self.n_done.item()) == self.N if self.fused else bool(self.done.all())

    def results(self) -> List[List[Tuple[float, List[int]]]]:
        k, F = self.k, self.F
        p = self.fin_p[:, :F]
        order = torch.sort(p, dim=1, descending=True, stable=True).indices[:, :k].cpu()
        p, ln, tk, n = p.cpu(), self.fin_len[:, :F].cpu(), self.fin_tok[:, :F].cpu(), self.fin_n.cpu()
        out = []
        for m in range(self.N):
            hyp = []
            for j in order[m].tolist():
                if j < int(n[m]):
                    hyp.append((float(p[m, j]), tk[m, j, : int(ln[m, j])].tolist()))
            out.append(hyp)
        return out


def _prefix_rows(prefix_ids: torch.Tensor, pair_of_molecule, N: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The bookkeeping of a prefill on the host: pair_of_molecule [N] names the (condition, prefix) pair every molecule starts from ->
    (it as int64 [N], dst int32 [Npairs]: the row that holds pair p's prefix = beam 0's row of the first molecule that starts from it)."""
    if prefix_ids.dim() != 2 or prefix_ids.shape[0] < 1 or prefix_ids.shape[1] < 1:
        raise ValueError(f"prefill: prefix_ids must be [Npairs, P] with P >= 1, got {tuple(prefix_ids.shape)}")
    pom = torch.as_tensor(pair_of_molecule).detach().cpu().to(torch.int64).reshape(-1)
    n_pairs = prefix_ids.shape[0]
    if pom.numel() != N or int(pom.min()) < 0 or int(pom.max()) >= n_pairs:
        raise ValueError(f"prefill: pair_of_molecule must name one of the {n_pairs} pairs for each of the {N} molecules")
    first = torch.full((n_pairs,), N, dtype=torch.int64)
    first.scatter_reduce_(0, pom, torch.arange(N, dtype=torch.int64), reduce="amin")
    if int(first.max()) >= N:
        raise ValueError("prefill: every pair must be the start of at least one molecule")
    return pom, (first * k).to(torch.int32)


def _decoder_warp(k: int, min_keep: int | None, base_embeds, memory=None, **controls) -> dict:
    """The warp a decoder carries, checked: check_warp's four controls (all at their defaults: NO_WARP) and min_keep (None: k), the tokens
    every row keeps whatever the truncation says -- k for the searches that draw k tokens per row, 1 for sample_distinct, whose rows
    contribute any number of candidates."""
    if memory is not None:
        raise ValueError("guidance contrasts a property condition with the all-masked one; a decoder with memory= (reaction prediction) "
                         "has no such baseline")
    min_keep = k if min_keep is None else int(min_keep)
    warp = check_warp(k=min_keep, **controls) or dict(NO_WARP)
    if base_embeds is None and warp["guidance"] != 1.0:
        raise ValueError(f"guidance={warp['guidance']} needs base_embeds, the encoded all-masked PV")
    return dict(warp, min_keep=min_keep)


class _Decoder:
    """What the searches ask of every decoder beyond the forward pass: the last mile of its logits.  `step` and `prefill` return what
    `finish` makes of the raw next-token logits -- a constrained search's grammar mask (`premask`, a SyntaxMask) first, on the RAW logits,
    then the warp the decoder carries (`carry_warp`) -- and with neither, the raw logits themselves: no launch, no tensor op."""
    cached = False                                       # one token per step against a K/V cache (CachedDecoder and its kin)
    premask = None
    warp, fused_warp = None, False                       # _decoder_warp's dict; the warp is ops.logit_warp (else warp_logits)
    warp_info = dict(NO_WARP, baseline_rows=0)           # what last_run records: the four controls, and the rows of the all-masked half
    xkv_once = None                                      # (cached: the cross-attention projections a later decoder on the same conditions takes)

    def carry_warp(self, warp: dict, baseline_rows: int = 0, fused: bool = False):
        self.warp, self.fused_warp = warp, fused
        self.warp_info = dict({f: warp[f] for f in NO_WARP}, baseline_rows=baseline_rows)

    def finish(self, lc: torch.Tensor, lu: torch.Tensor | None = None, by: str = "row") -> torch.Tensor:
        """Raw logits lc [n, V] -- and lu, those of the rows' all-masked twins -- -> what the search reads.  by: SyntaxMask's."""
        if self.premask is not None:                     # both halves alike: masking lc alone would be wrong for guidance <= 0
            self.premask(lc, lu, by=by)
        w = self.warp
        if w is None:
            return lc
        if self.fused_warp:
            return ops.logit_warp(lc, lu, w=w["guidance"], temperature=w["temperature"], top_k=w["top_k"], top_p=w["top_p"], min_keep=w["min_keep"])
        return warp_logits(lc.float(), None if lu is None else lu.float(), **w)


class RecomputeDecoder(_Decoder):
    """Step function with the reference's cost model: re-runs the whole prefix of every beam through the module API
    (`model.text_encoder(..., is_decoder=True, return_logits=True)`), so it works with the CPU oracle as well."""

    def __init__(self, model, prop_embeds: torch.Tensor, k: int, Lmax: int):
        self.m, self.k = model, k
        self.kv = prop_embeds.repeat_interleave(k, dim=0)
        self.device = prop_embeds.device
        self.tok = torch.zeros(self.kv.shape[0], Lmax, dtype=torch.long, device=self.device)

    def _forward(self, ids: torch.Tensor, t: int) -> torch.Tensor:
        self.tok[:, t] = ids
        text = self.tok[:, : t + 1]
        return self.m.text_encoder(text, attention_mask=torch.ones_like(text), encoder_hidden_states=self.kv,
                                   encoder_attention_mask=torch.ones(self.kv.shape[:-1], dtype=torch.long, device=self.device),
                                   return_dict=True, is_decoder=True, return_logits=True)[:, -1, :]

    def step(self, ids: torch.Tensor, t: int) -> torch.Tensor:
        return self.finish(self._forward(ids, t))

    def prefill(self, prefix_ids: torch.Tensor, pair_of_molecule, by_steps: bool = False) -> torch.Tensor:
        """CachedDecoder.prefill for the whole-prefix forward: the rows are seeded with their prefix tokens -> logits [Npairs, V] for
        position P (one forward over all rows; by_steps means nothing here)."""
        pom, dst = _prefix_rows(prefix_ids, pair_of_molecule, self.tok.shape[0] // self.k, self.k)
        rows = prefix_ids.to(self.device).long()[pom.to(self.device)].repeat_interleave(self.k, dim=0)        # [N*k, P]
        P = rows.shape[1]
        self.tok[:, :P - 1] = rows[:, :P - 1]
        return self.finish(self._forward(rows[:, P - 1], P - 1)[dst.to(self.device).long()], by="pair")

    def reorder(self, parent: torch.Tensor, t: int):
        N, k = parent.shape
        L = self.tok.shape[1]
        self.tok = self.tok.view(N, k, L).gather(1, parent[:, :, None].expand(N, k, L)).reshape(N * k, L)


def _cross_kv(eng, bert_pfx: str, c, rows: torch.Tensor) -> dict:
    """Keys | values of the cross-attention of every fusion layer, projected once from `rows` (bf16 [M, H]): {layer: bf16 [M, 2H]}."""
    P, out = eng.P, {}
    for l in range(c.fusion_layer, c.num_hidden_layers):
        pf = f"{bert_pfx}encoder.layer.{l}.crossattention.self."
        out[l] = ops.gemm_nt(rows, P.fused(pf, ("key", "value"), "weight"), eng._new(rows.shape[0], 2 * c.hidden_size),
                             bias=P.fused(pf, ("key", "value"), "bias", what="w"))
    return out


class CachedDecoder(_Decoder):
    """One new token per beam per step on the HIP engine: per-layer self-attention K/V cache [R, Lmax, H] that is never
    moved (the ancestry table `anc[r, j]` names the cache row holding position j of row r's hypothesis), cross-attention
    K/V projected once per molecule and shared by its k beams (cache slots sketched at
    xbert.py:291-295,480,1344-1348).  Carrying a warp (`carry_warp`: temperature, top-k, nucleus -- no guidance, which needs the second
    half of GuidedDecoder) it warps with the kernel where the one-launch beam step runs (k <= 8, V <= 512, FUSED_BEAM_STEP)."""
    cached = True

    def __init__(self, model, prop_embeds: torch.Tensor | None, k: int, Lmax: int, repeat: int = 1, xkv: dict | None = None, memory: dict | None = None,
                 src: torch.Tensor | None = None):
        """repeat: decode `repeat` molecules per row of prop_embeds (generation of many samples from one PV: the cross-attention keys /
        values are projected once per row and copied).  xkv: the projections of an earlier decoder on the same prop_embeds (`xkv_once`).
        src (host int64 [N], instead of repeat): molecule n decodes against row src[n] of prop_embeds -- `repeat` for any assignment
        (GuidedDecoder: N molecules on their conditions, N more on the one all-masked row).
        memory (instead of prop_embeds): a masked, variable-length cross-attention memory, one source per molecule -- dict(N, xkv = {layer:
        bf16 [M, 2H] keys | values of token-major rows}, row0 / len = int32 [N] first row and length of every source, Lmax = the longest
        length allowed) -- read through spmm_decode_xattn; it is never moved: `compact` gathers the molecule -> source index alone."""
        from .engine import BF
        eng = model.engine
        self.eng, self.P, self.c, self.k = eng, eng.P, model.cfg.text, k
        self.pfx = "text_encoder."
        c, dev = self.c, model.device_
        self.device = dev
        self.mem, self.kv_seq = memory, None             # kv_seq: after compact(), the source of every molecule still decoded (None: its own)
        if memory is not None:
            assert prop_embeds is None and repeat == 1 and xkv is None
            N, Lkv, H = memory["N"], memory["Lmax"], c.hidden_size
        else:
            N, Lkv, H = prop_embeds.shape
        self.src = None if src is None else torch.as_tensor(src).detach().cpu().to(torch.int64).reshape(-1)
        if self.src is not None:
            assert memory is None and repeat == 1 and int(self.src.min()) >= 0 and int(self.src.max()) < N
            N = self.src.numel()
        N *= repeat
        check_positions(Lmax)
        assert H == c.hidden_size and c.hidden_size // c.num_attention_heads == 64
        self.N, self.R, self.Lmax, self.Lp, self.H = N, N * k, Lmax, Lkv, H
        # head-major cache [R, nH, Lmax, 64]: the positions of a (row, head) are one contiguous 128-B-per-key stream for the wave that reads them
        self.kc = [torch.empty(self.R, c.num_attention_heads, Lmax, 64, dtype=BF, device=dev) for _ in range(c.num_hidden_layers)]
        self.vc = [torch.empty(self.R, c.num_attention_heads, Lmax, 64, dtype=BF, device=dev) for _ in range(c.num_hidden_layers)]
        self.anc = torch.arange(self.R, dtype=torch.int32, device=dev)[:, None].repeat(1, Lmax).contiguous()
        self.rows = torch.arange(self.R, dtype=torch.int32, device=dev)
        self.cols = torch.arange(Lmax, device=dev)
        self.rowmap = None                               # after compact(): cache row of every beam row still decoded (None: the row itself)
        self.cond, self.repeat = prop_embeds, repeat     # (prefill: the conditions the fusion layers of the packed pass are bound to)
        if memory is not None:
            self.xkv_once = self.xkv = memory["xkv"]
            return
        if xkv is None:
            xkv = _cross_kv(eng, self.pfx + "bert.", c, prop_embeds.to(dev).to(BF).reshape(-1, H).contiguous())
        self.xkv_once = xkv                              # per row of prop_embeds
        self._expand_xkv(xkv)

    def _expand_xkv(self, xkv: dict):
        """self.xkv: the keys | values every molecule of the batch reads, one [Lp, 2H] block per molecule, from the per-condition `xkv`."""
        Lkv, H = self.Lp, self.H
        if self.src is not None:
            pick = self.src.to(self.device)
            self.xkv = {l: KV.view(-1, Lkv, 2 * H).index_select(0, pick).reshape(-1, 2 * H) for l, KV in xkv.items()}
        else:
            self.xkv = {l: (KV.view(-1, Lkv, 2 * H).repeat_interleave(self.repeat, dim=0).reshape(-1, 2 * H) if self.repeat > 1 else KV)
                        for l, KV in xkv.items()}

    def carry_warp(self, warp: dict, baseline_rows: int = 0):
        super().carry_warp(warp, baseline_rows, fused=bool(FUSED_BEAM_STEP and self.k <= 8 and self.c.vocab_size <= 512))

    def search_tables(self) -> Tuple[torch.Tensor, torch.Tensor | None]:
        """(anc, rowmap) as the search's beam step updates / reads them: the rows of the beams it keeps books for."""
        return self.anc, self.rowmap

    @torch.no_grad()
    def compact(self, keep: torch.Tensor):
        """Drop every molecule but the batch slots `keep` (int64, ascending) from the decoded batch: activations shrink to len(keep) * k
        rows.  The K/V caches are NOT moved -- the ancestry table keeps naming the cache rows, and `rowmap` says where a surviving row
        writes its next position -- only the ancestry rows and the (per-molecule) cross-attention keys / values are gathered."""
        k, L, Lp = self.k, self.Lmax, self.Lp
        cur = self.rows if self.rowmap is None else self.rowmap
        self.rowmap = cur.view(self.N, k)[keep].reshape(-1).contiguous()
        self.anc = self.anc.view(self.N, k, L)[keep].reshape(-1, L).contiguous()
        if self.mem is not None:                         # the memory stays where it is: only the molecule -> source index is gathered
            cur = torch.arange(self.N, dtype=torch.int32, device=self.device) if self.kv_seq is None else self.kv_seq
            self.kv_seq = cur[keep].contiguous()
        else:
            self._compact_xkv(keep)
        self.N = int(keep.numel())
        self.R = self.N * k

    def _compact_xkv(self, keep: torch.Tensor):
        """`compact` for the per-molecule cross-attention keys | values (self.N is still the batch before the compaction)."""
        for l, KV in self.xkv.items():
            self.xkv[l] = KV.view(self.N, self.Lp, KV.shape[1])[keep].reshape(-1, KV.shape[1]).contiguous()

    def _cross_attn(self, l: int, q: torch.Tensor, ctx: torch.Tensor):
        """Newest-position cross-attention of fusion layer l: queries q [R, H] -> ctx, every molecule's k beams on its own keys | values."""
        H, nH, KV = self.H, self.c.num_attention_heads, self.xkv[l]
        if self.mem is None:
            ops.decode_attn(q, KV[:, :H], KV[:, H:], ctx, nH=nH, Lkv=self.Lp, seq_stride=self.Lp * 2 * H, tok_stride=2 * H, kv_div=self.k, group=self.k)
        else:
            ops.decode_xattn(q, KV[:, :H], KV[:, H:], ctx, nH=nH, kv_seq=self.kv_seq, kv_row0=self.mem["row0"], kv_len=self.mem["len"],
                             Lkv_max=self.Lp, group=self.k)

    @torch.no_grad()
    def step(self, ids: torch.Tensor, t: int, t_dev: torch.Tensor | None = None) -> torch.Tensor:
        """ids [R]: the token at position t of every beam -> fp32 logits [R, V] for position t + 1 (`finish` of the raw ones).
        t_dev (int32 [1], device): the position comes from device memory instead (t is then ignored), which makes the whole
        launch sequence independent of the step -- capturable once as a hipGraph and replayed (beam_search_batched(graph=True))."""
        return self.finish(self._forward(ids, t, t_dev))

    @torch.no_grad()
    def _forward(self, ids: torch.Tensor, t: int, t_dev: torch.Tensor | None = None) -> torch.Tensor:
        """`step` up to the raw logits, on all R rows the decoder holds."""
        P, c, R, H, nH, new = self.P, self.c, self.R, self.H, self.c.num_attention_heads, self.eng._new
        bp = self.pfx + "bert."
        # residual sublayers: the engine's (inference: no tape, dropout off -- the row kernel then never reads the seed)
        sub = functools.partial(self.eng._proj_ln, X32=None, save=False, eps=c.layer_norm_eps, ph=0.0, salt=0)
        x = new(R, H)
        ops.embed_step_ln_fwd(ids.to(torch.int32).contiguous(), t, x, pos_ptr=t_dev, word=P.w(bp + "embeddings.word_embeddings.weight"),
                              pos=P.w(bp + "embeddings.position_embeddings.weight"), type0=P.w(bp + "embeddings.token_type_embeddings.weight"),
                              gamma=P.w(bp + "embeddings.LayerNorm.weight"), beta=P.w(bp + "embeddings.LayerNorm.bias"), eps=c.layer_norm_eps)
        for l in range(c.num_hidden_layers):
            lp = f"{bp}encoder.layer.{l}."
            pf = lp + "attention."
            QKV = new(R, 3 * H)
            ops.gemm_nt(x, P.fused(pf + "self.", ("query", "key", "value"), "weight"), QKV,
                        bias=P.fused(pf + "self.", ("query", "key", "value"), "bias", what="w"))
            ctx = new(R, H)                       # (the launch also moves the new key / value rows into the cache)
            ops.decode_attn(QKV[:, :H], self.kc[l], self.vc[l], ctx, nH=nH, Lkv=self.Lmax if t_dev is not None else t + 1,
                            seq_stride=self.Lmax * H, tok_stride=64, head_stride=self.Lmax * 64, anc=self.anc, group=self.k, t_ptr=t_dev, knew=QKV[:, H:2 * H], vnew=QKV[:, 2 * H:],
                            rowmap=self.rowmap)
            a = sub(pf + "output.", ctx, x)[0]
            if l >= c.fusion_layer:
                pf = lp + "crossattention."
                q = new(R, H)
                ops.gemm_nt(a, P.wb(pf + "self.query.weight"), q, bias=P.w(pf + "self.query.bias"))
                self._cross_attn(l, q, ctx)
                a = sub(pf + "output.", ctx, a)[0]
            h = new(R, c.intermediate_size)
            ops.gemm_nt(a, P.wb(lp + "intermediate.dense.weight"), h, bias=P.w(lp + "intermediate.dense.bias"), epi=ops.EPI_GELU)
            x = sub(lp + "output.", h, a)[0]
        logits, _ = self.eng.lm_head_fwd(self.pfx, c, x, False)
        return logits

    @torch.no_grad()
    def prefill(self, prefix_ids: torch.Tensor, pair_of_molecule, by_steps: bool = False) -> torch.Tensor:
        """Start every molecule from a prefix instead of [CLS] alone: prefix_ids int [Npairs, P] (position 0 = [CLS]), one row per
        (condition, prefix) pair; pair_of_molecule [N] names the pair molecule n starts from, and the pair's condition is that molecule's
        (one pair per molecule, or -- repeat > 1, many samples of one PV -- one pair for all).  -> fp32 logits [Npairs, V] for position P;
        afterwards `step(ids, P)` continues.  Call it on a fresh decoder (before any step / compact).
        One packed pass over the P positions of every pair, as score._decode_scores runs it (eval mode, no tape): the unimodal layers once
        per DISTINCT prefix, the fusion layers per pair, each bound to its condition's keys | values (`xkv_once`: nothing is projected
        again); every layer's self-attention K | V go from the Q|K|V projection into ONE cache row per pair (ops.kv_prefill), beam 0's
        row of the first molecule that starts from the pair, and `anc[:, :P]` of every row names that row: the cache is never copied per
        beam, and positions that all beams of a molecule read from one row are the attention kernel's shared-key fast path.  The LM head
        runs on the pairs' last-position rows only.
        by_steps=True: the twin on existing kernels only -- the prefix fed through the raw step position by position on all N*k rows,
        identity ancestry: the parity yard-stick and the timing baseline, not meant to be fast.
        Either way the raw logits of position P are finished once, by pair: a grammar mask reads the prefixes and nothing before them."""
        return self.finish(self._prefill(prefix_ids, pair_of_molecule, by_steps), by="pair")

    @torch.no_grad()
    def _prefill(self, prefix_ids: torch.Tensor, pair_of_molecule, by_steps: bool) -> torch.Tensor:
        """`prefill` up to the raw logits [Npairs, V]."""
        from .engine import BF, KVSource, Group, Batch
        if self.mem is not None:
            raise ValueError("prefill: prompted decoding is for the PV decoder; a decoder with memory= (reaction prediction) has none")
        eng, c, k, H, dev = self.eng, self.c, self.k, self.H, self.device
        pom, dst = _prefix_rows(prefix_ids, pair_of_molecule, self.N, k)
        n_pairs, P = prefix_ids.shape
        if P >= self.Lmax:
            raise ValueError(f"prefill: a prefix of {P} tokens does not fit a cache of Lmax={self.Lmax} positions")
        ids_h = prefix_ids.detach().cpu().to(torch.int64)
        if by_steps:
            rows = ids_h[pom].repeat_interleave(k, dim=0).to(dev)               # [N*k, P]
            for j in range(P):
                logits = self._forward(rows[:, j].contiguous(), j)
            return logits[dst.to(dev).long()]
        eng.train_mode = False
        TP, f, n = self.pfx + "bert.", c.fusion_layer, c.num_hidden_layers
        i32 = lambda a: a.to(torch.int32).contiguous().to(dev)                  # noqa: E731
        uniq, inv = torch.unique(ids_h, dim=0, return_inverse=True)
        U = uniq.shape[0]
        dst_d, len_d = dst.to(dev), torch.full((n_pairs,), P, dtype=torch.int32, device=dev)
        row0_lo, row0_hi = i32(inv * P), i32(torch.arange(n_pairs) * P)          # first source row of pair p: layers < f, layers >= f

        def fill(row0, l, QKV):
            ops.kv_prefill(QKV[:, H:2 * H], QKV[:, 2 * H:], row0, len_d, dst_d, self.kc[l], self.vc[l])

        # ---- the unimodal layers, causal, once per distinct prefix (equal lengths: the dense rows are the packed rows)
        x, _ = eng.embed_text(TP, c, i32(uniq), U, P, False)
        text, _, _ = eng.stack_fwd(TP, c, range(0, f), False, x, Batch([Group(0, U, P, None, 0)]), False, kv_tap=functools.partial(fill, row0_lo))
        # ---- the fusion layers: the pairs' query rows, causal, pair p bound to the condition of its first molecule
        if U != n_pairs or not torch.equal(inv, torch.arange(n_pairs)):
            text = text.index_select(0, (inv[:, None] * P + torch.arange(P)[None, :]).reshape(-1).to(dev))
        Lp = self.Lp
        proj = {f"{TP}encoder.layer.{l}.crossattention": KV for l, KV in self.xkv_once.items()}
        cond = self.cond.to(dev).to(BF).reshape(-1, H).contiguous()
        src = KVSource(cond, cond.shape[0] // Lp, Lp, proj=proj)
        mol0 = dst.long() // k                                                   # first molecule of every pair: the pair's condition is its
        g = Batch([Group(0, n_pairs, P, None, 0).bind(src, i32(mol0 // self.repeat if self.src is None else self.src[mol0]), 0)])
        y, _, _ = eng.stack_fwd(TP, c, range(f, n), True, text, g, False, kv_tap=functools.partial(fill, row0_hi))
        self.anc[:, :P] = dst_d[pom.to(dev)].repeat_interleave(k)[:, None]
        last = y.index_select(0, (torch.arange(n_pairs) * P + P - 1).to(dev))
        logits, _ = eng.lm_head_fwd(self.pfx, c, last, False)
        return logits

    @torch.no_grad()
    def reorder(self, parent: torch.Tensor, t):
        """New beam b of molecule n continues old beam parent[n, b]; positions < t are inherited, position t and everything behind it
        is its own.  t: int, or int64 [1] in device memory (graph replay).  The table is updated in place: its address is static."""
        N, k, L = self.N, self.k, self.Lmax
        anc = self.anc.view(N, k, L).gather(1, parent[:, :, None].expand(N, k, L)).reshape(N * k, L)
        torch.where(self.cols >= t, self.rows[:, None], anc, out=self.anc)


class GuidedDecoder(CachedDecoder):
    """CachedDecoder with classifier-free guidance against the decoder's own all-masked prediction (base_embeds) in its warp, next to
    temperature, top-k and nucleus truncation (warp_logits' rules).
    Guidance runs both conditions in ONE set of launches: the decoder holds 2N molecules, rows [0, R) on their conditions and rows
    [R, 2R) on the baseline (R = N * k), the all-masked PV encoded and projected once (base_embeds [1, Lp, H]: with every property
    masked the encoding does not depend on the PV) and its keys | values shared by all N baseline molecules: their cross-attention is a
    second launch per fusion layer that reads the one block with sequence stride 0.
    Both halves are fed the same tokens; ops.logit_warp combines the two halves of the logits (lu = lc + R * ld) in place, and the search
    sees [R, V] logits, anc[:R] and rowmap[:R] (`search_tables`): BeamBook, the beam step and the noise know nothing of the second half.
    The baseline half's ancestry is the mirror anc[R + r, j] = anc[r, j] + R0 (R0: the uncompacted R; cache rows keep their indices
    under compaction, so the offset is constant), refreshed by one small launch at the head of every step.
    The scores the search records are log-probabilities of the warped distribution, renormalised over the kept tokens.
    A warp without guidance needs no second half: it is CachedDecoder's own (`carry_warp`; make_decoder)."""

    def __init__(self, model, prop_embeds: torch.Tensor, k: int, Lmax: int, repeat: int = 1, xkv: dict | None = None, memory: dict | None = None, *,
                 base_embeds: torch.Tensor | None = None, guidance: float = 1.0, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                 min_keep: int | None = None):
        """min_keep: _decoder_warp's."""
        warp = _decoder_warp(k, min_keep, base_embeds, memory, guidance=guidance, temperature=temperature, top_k=top_k, top_p=top_p)
        if base_embeds is None:
            raise ValueError("a guided decoder needs base_embeds, the encoded all-masked PV, for its second half")
        Nc = prop_embeds.shape[0]
        conds = torch.cat([prop_embeds, base_embeds[:1].to(prop_embeds.device).to(prop_embeds.dtype)], dim=0)
        src = torch.cat([torch.arange(Nc).repeat_interleave(repeat), torch.full((Nc * repeat,), Nc, dtype=torch.int64)])
        super().__init__(model, conds, k, Lmax, xkv=xkv, src=src)
        self.R0 = self.R // 2                                             # beam rows of the search before any compaction
        self.carry_warp(warp, baseline_rows=self.R0)

    def finish(self, logits: torch.Tensor, lu=None, by: str = "row") -> torch.Tensor:
        """Raw fp32 [2n, V], the conditioned rows and then their baseline twins (lu is not passed: it is the second half) -> warped [n, V],
        in place where the kernel runs."""
        n = logits.shape[0] // 2
        return super().finish(logits[:n], logits[n:], by)

    def _expand_xkv(self, xkv: dict):
        """The conditioned half as CachedDecoder expands it; the baseline half reads ONE copy, the all-masked row's projection."""
        Lp, H, n = self.Lp, self.H, self.N // 2
        pick = self.src[:n].to(self.device)
        self.xkv = {l: KV.view(-1, Lp, 2 * H).index_select(0, pick).reshape(-1, 2 * H) for l, KV in xkv.items()}
        self.xkv_base = {l: KV.view(-1, Lp, 2 * H)[-1] for l, KV in xkv.items()}        # [Lp, 2H] views of xkv_once

    def _compact_xkv(self, keep: torch.Tensor):
        n = self.N // 2                                                   # (keep = the kept slots of the first half, then their twins)
        for l, KV in self.xkv.items():
            self.xkv[l] = KV.view(n, self.Lp, KV.shape[1])[keep[:keep.numel() // 2]].reshape(-1, KV.shape[1]).contiguous()

    def _cross_attn(self, l: int, q: torch.Tensor, ctx: torch.Tensor):
        """Two launches: the conditioned rows on their molecules' keys | values, the baseline rows all on the one all-masked block
        (sequence stride 0: every molecule's "own" block is block 0)."""
        H, nH, R, KV, B = self.H, self.c.num_attention_heads, self.R // 2, self.xkv[l], self.xkv_base[l]
        ops.decode_attn(q[:R], KV[:, :H], KV[:, H:], ctx[:R], nH=nH, Lkv=self.Lp, seq_stride=self.Lp * 2 * H, tok_stride=2 * H, kv_div=self.k, group=self.k)
        ops.decode_attn(q[R:], B[:, :H], B[:, H:], ctx[R:], nH=nH, Lkv=self.Lp, seq_stride=0, tok_stride=2 * H, kv_div=self.k, group=self.k)

    def search_tables(self):
        R = self.R // 2
        return self.anc[:R], (None if self.rowmap is None else self.rowmap[:R])

    @torch.no_grad()
    def step(self, ids: torch.Tensor, t: int, t_dev: torch.Tensor | None = None) -> torch.Tensor:
        """ids [R]: the token at position t of every beam of the search -> warped fp32 logits [R, V] for position t + 1."""
        R = self.R // 2
        assert ids.numel() == R, (ids.shape, R)
        torch.add(self.anc[:R], self.R0, out=self.anc[R:])               # the mirror: what the beam step did to the first half since the last step
        ids = ids.to(torch.int32)
        return self.finish(self._forward(torch.cat([ids, ids]), t, t_dev))

    @torch.no_grad()
    def compact(self, keep: torch.Tensor):
        """`keep` (slots of the search's batch) -> the same molecules of both halves."""
        super().compact(torch.cat([keep, keep + self.N // 2]))

    @torch.no_grad()
    def reorder(self, parent: torch.Tensor, t):
        super().reorder(torch.cat([parent, parent], dim=0), t)

    @torch.no_grad()
    def _prefill(self, prefix_ids: torch.Tensor, pair_of_molecule, by_steps: bool) -> torch.Tensor:
        """Every (condition, prefix) pair gets a baseline twin (pair p + Npairs, the start of the baseline molecules of p's molecules): the
        unimodal layers still run once per distinct prefix, the twin's cache row is the pair's + R0 -- what the mirror expects (by_steps:
        a fresh decoder's identity ancestry is its own mirror) -- and the raw logits come back as `finish` reads them, pairs then twins."""
        pom, _ = _prefix_rows(prefix_ids, pair_of_molecule, self.N // 2, self.k)
        return super()._prefill(torch.cat([prefix_ids, prefix_ids], dim=0), torch.cat([pom, pom + prefix_ids.shape[0]]), by_steps)


class GuidedRecompute(_Decoder):
    """The warping decoders' twin on whole-prefix forwards (RecomputeDecoder: any model with the module API, the CPU oracle included): one
    decoder per condition -- they return raw logits, carrying neither mask nor warp -- and warp_logits.  The yard-stick of the cached route."""

    def __init__(self, model, prop_embeds: torch.Tensor, k: int, Lmax: int, *, base_embeds: torch.Tensor | None = None, guidance: float = 1.0,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, min_keep: int | None = None):
        warp = _decoder_warp(k, min_keep, base_embeds, guidance=guidance, temperature=temperature, top_k=top_k, top_p=top_p)
        self.k, self.device = k, prop_embeds.device
        self.halves = [RecomputeDecoder(model, prop_embeds, k, Lmax)]
        if base_embeds is not None:
            self.halves.append(RecomputeDecoder(model, base_embeds[:1].expand(prop_embeds.shape[0], -1, -1), k, Lmax))
        self.carry_warp(warp, baseline_rows=(len(self.halves) - 1) * prop_embeds.shape[0] * k)

    def step(self, ids: torch.Tensor, t: int) -> torch.Tensor:
        return self.finish(*[d.step(ids, t) for d in self.halves])

    def prefill(self, prefix_ids: torch.Tensor, pair_of_molecule, by_steps: bool = False) -> torch.Tensor:
        return self.finish(*[d.prefill(prefix_ids, pair_of_molecule) for d in self.halves], by="pair")

    def reorder(self, parent: torch.Tensor, t: int):
        for d in self.halves:
            d.reorder(parent, t)


PAD_ID = 0
DECODE_MAXL = 256              # positions the decode kernels hold (spmm_decode_attn, spmm_beam_step, spmm_gumbel_noise)


def check_positions(Lmax: int, P: int | None = None) -> int:
    """The positions a search holds, Lmax = P + max_steps + 2 (P given: spelled out in the message) -> Lmax, or ValueError beyond DECODE_MAXL."""
    if Lmax > DECODE_MAXL:
        how = "" if P is None else f"P + max_steps + 2 = {P} + {Lmax - P - 2} + 2 = "
        raise ValueError(f"{how}{Lmax} positions exceed the {DECODE_MAXL} the decode kernels hold (max_steps counts positions after the prefix)")
    return Lmax


def check_prefix(prefix, N: int, vocab_size: int | None, max_steps: int) -> torch.Tensor | None:
    """The `prefix` argument of the searches -> int64 [N or 1, P] on the host, or None for no prefix / [CLS] alone (today's start).
    prefix: ints, [P] (one prefix for all molecules) or [N, P]; one length per call."""
    if prefix is None:
        return None
    if not torch.is_tensor(prefix):
        rows = list(prefix)
        nested = [isinstance(r, (list, tuple)) or (torch.is_tensor(r) and r.dim() > 0) for r in rows]
        if any(nested):
            if not all(nested) or len({len(r) for r in rows}) != 1:
                raise ValueError("prefix: prefixes of different lengths in one call; group the molecules by prefix length and call once per length")
            rows = [[int(t) for t in r] for r in rows]
        prefix = torch.tensor(rows, dtype=torch.int64)
    if prefix.dtype.is_floating_point or prefix.dtype == torch.bool:
        raise ValueError(f"prefix: token ids must be integers, got {prefix.dtype}")
    p = prefix.detach().cpu().to(torch.int64)
    if p.dim() == 1:
        p = p[None, :]
    elif p.dim() != 2:
        raise ValueError(f"prefix: [P] or [N, P] token ids, got {p.dim()} dimensions")
    if p.shape[1] < 1 or p.shape[0] not in (1, N):
        raise ValueError(f"prefix: shape {tuple(p.shape)} is neither [P] nor [N, P] with N = {N} molecules and P >= 1")
    if bool((p[:, 0] != CLS_ID).any()):
        raise ValueError(f"prefix: the first token must be [CLS] ({CLS_ID})")
    if bool(((p == SEP_ID) | (p == PAD_ID)).any()):
        raise ValueError(f"prefix: [SEP] ({SEP_ID}) or PAD ({PAD_ID}) inside a prefix")
    if int(p.min()) < 0 or (vocab_size is not None and int(p.max()) >= vocab_size):
        raise ValueError(f"prefix: token id {int(p.max()) if int(p.min()) >= 0 else int(p.min())} outside the vocabulary of {vocab_size}")
    check_positions(p.shape[1] + max_steps + 2, p.shape[1])
    return None if p.shape[1] == 1 else p


def _vocab_size(model) -> int | None:
    return getattr(getattr(getattr(model, "cfg", None), "text", None), "vocab_size", None)


@torch.no_grad()
def beam_search_batched(model, props: torch.Tensor, k: int = 5, max_steps: int = 100, cached: bool | None = None,
                        sync_every: int = 4, prop_mask: torch.Tensor | None = None, stochastic: bool = False,
                        generator=None, graph: bool | None = None, compact: bool = True, seed: int | None = None,
                        mol_base: int = 0, prefix=None, prefill: bool = True, guidance: float = 1.0, temperature: float = 1.0, top_k: int = 0,
                        top_p: float = 1.0, syntax=None) -> List[List[Tuple[float, List[int]]]]:
    """The reference's beam search for N molecules at once (props [N,53]); result[n] is what the one-molecule search
    (oracle/decode_oracle.py::beam_search) returns for props[n].
    cached=True (default on the HIP model) decodes one token per step against the K/V cache; cached=False re-runs the prefix
    through the module API (any model exposing it, e.g. the CPU oracle).  prop_mask: properties to leave unspecified
    (encode_properties).  stochastic=True draws the k candidates of every beam from the next-token distribution instead of
    taking the k most probable (d_pv2smiles_single.py:37-40).  Without `seed` the draws are torch.multinomial's, from `generator`, on the
    tensor-op bookkeeping.  With `seed` every position -- position 0 from [CLS] included (t = 0, b = 0) -- draws by Gumbel-top-k from
    counter noise keyed by (seed, mol_base + n, position, beam, token) (ops.gumbel_noise / gumbel_noise_host): molecule mol_base + n gets
    the same draws whatever batch it is decoded in, the search runs on the one-launch beam step under the same conditions as the
    deterministic one, and finished molecules are dropped (`compact`) as they are there.
    graph=True (cached, deterministic) captures one decode position -- ~230 launches -- as a hipGraph and replays it: the per-position
    host cost drops from ~2.3 ms of launch overhead to one graph launch, which is what small batches are bound by.  Replay is opt-in:
    graph=None (default) and graph=False are the eager loop.  Every call re-captures its launches (a graph is tied to this call's buffers),
    capture is process-global on the capture stream's device -- another thread touching the GPU meanwhile aborts it -- and a replayed
    graph cannot drop finished molecules; it gains 7 % at 100 beam rows and nothing from 500 on (GRAPH_BELOW_ROWS).  A sampled search
    (seeded or not) stays eager whatever `graph` says.  compact=True (eager fused path): finished
    molecules are dropped from the batch as the search goes (same results; the reference decodes one molecule at a time and simply stops).
    prefix: the beginning of every molecule -- token ids [P] (one prefix for all molecules) or [N, P], a list or a tensor, starting with
    [CLS], no [SEP] or PAD inside, one length per call (ValueError otherwise: the caller groups molecules by prefix length).  Every
    hypothesis then starts with its prefix, its score counts the generated tokens only, and max_steps counts positions after the prefix
    (P + max_steps + 2 <= 256).  The noise of a seeded search is keyed by the absolute position, so the first pick draws at P - 1.
    prefill=True: the prefix goes through the decoder once, in one packed pass, into one cache row per molecule that all its beams read
    (CachedDecoder.prefill); prefill=False: it is stepped through position by position on every beam row (the twin on the existing
    kernels).  cached=False seeds the whole-prefix forward with the tokens.  A search with a prefix stays eager whatever `graph` says.
    prefix=None, or [CLS] alone, is the search without a prefix, unchanged.
    guidance, temperature, top_k, top_p: the distribution every position picks or draws from (warp_logits' rules, min_keep = k), the first
    pick from [CLS] or from the prefix logits included, on the deterministic search and the sampled ones alike.  guidance w != 1 is
    classifier-free guidance, log p~ = log p_u + w (log p_c - log p_u), between the search's condition (props, prop_mask) and the all-masked
    PV -- pretraining masks every property with probability 0.5, so the one decoder is also the baseline; w > 1 pushes towards the
    requested properties, w = 0 is the all-masked model.  Both conditions run as two halves of one set of launches (GuidedDecoder;
    cached=False: two whole-prefix decoders and warp_logits).  The scores returned are log-probabilities of the warped distribution,
    renormalised over the kept tokens.  The seeded draws stay keyed by (seed, global molecule, absolute position, beam, token).
    ValueError before anything runs for temperature <= 0, top_p outside (0, 1], top_k < 0 or in [1, k), a non-finite guidance.  With any
    of the four set the search stays eager whatever `graph` says; with all four at their defaults (guidance = 1 never builds the
    baseline) it is the search without them, launch for launch.  last_run records the four and baseline_rows (0 or N*k).
    syntax: None / False -- the search as it is, launch for launch -- or True (the grammar table is built from model.tokenizer) or a
    smiles_syntax.SyntaxTable: every position, the first pick included, chooses among the tokens that can follow the beam's own history in
    a well-formed SMILES string that still ends by the last position (smiles_syntax.py: grammar, cost, invariant; SYNTAX ONLY -- no
    elements, valence, aromaticity, `%nn`).  The mask goes on the raw logits before guidance and truncation read them (on both halves of
    a guided decoder); one launch per position (ops.smiles_mask) wherever the one-launch beam step runs, smiles_syntax.allowed on the
    host elsewhere.  A beam with fewer than k allowed tokens takes masked ones too: those hypotheses score <= -1e29 and are not
    returned (last_run["dropped_masked"]); the scores returned are renormalised over the allowed (and kept) tokens.  ValueError before
    anything runs when the model has no tokenizer, the vocabulary lacks a closing piece, or the prefix rejects or cannot be closed in
    max_steps tokens.  A constrained search stays eager whatever `graph` says."""
    warp = check_warp(guidance, temperature, top_k, top_p, k)
    if cached is None:
        cached = hasattr(model, "engine")
    prefix = check_prefix(prefix, props.shape[0], _vocab_size(model), max_steps)
    table = syntax_table(model, syntax, prefix, max_steps)
    prop_embeds = encode_properties(model, props, prop_mask)
    if cached:
        model.engine.train_mode = False
    N = prop_embeds.shape[0]
    P = 1 if prefix is None else prefix.shape[1]
    base = _baseline_embeds(model, props[:1]) if warp is not None and warp["guidance"] != 1.0 else None      # (guidance = 1 never builds it)
    dec = make_decoder(model, prop_embeds, k, P + max_steps + 2, cached, warp, base_embeds=base)
    if prefix is not None:
        prefix = prefix.expand(N, P)                     # one (PV, prefix) pair per molecule; equal prefixes share the unimodal layers
    return _search(model, dec, N, k=k, max_steps=max_steps, sync_every=sync_every, stochastic=stochastic, generator=generator,
                   graph=bool(graph), compact=compact, seed=seed, mol_base=mol_base, prefix=prefix, pair_of_molecule=range(N), prefill=prefill,
                   table=table)


def _baseline_embeds(model, pv: torch.Tensor) -> torch.Tensor:
    """The baseline of guidance: a PV with every property masked, encoded -> [1, Lp, H] (the values of pv do not enter it)."""
    pv = pv.reshape(1, -1)
    return encode_properties(model, pv, torch.ones(1, pv.shape[1], device=pv.device))


def make_decoder(model, prop_embeds: torch.Tensor, k: int, Lmax: int, cached: bool, warp: dict | None, *, base_embeds: torch.Tensor | None = None,
                 repeat: int = 1, xkv: dict | None = None, min_keep: int | None = None):
    """The decoder of a search over `repeat` molecules per row of prop_embeds, k rows each: on the K/V cache (cached) or on whole-prefix
    forwards, carrying `warp` (check_warp's result; None: none) with min_keep (_decoder_warp's), in two halves when base_embeds (the
    encoded all-masked PV) asks for guidance.  xkv: `xkv_once` of an earlier decoder of this call on the same conditions (None from a
    whole-prefix one, which projects nothing).  The searches know a decoder by `step`, `prefill`, `reorder` / `search_tables`,
    `compact`, `premask`, `warp`, `warp_info`, `cached` and `xkv_once`, never by its class."""
    if not cached:
        pe = prop_embeds if repeat == 1 else prop_embeds.repeat_interleave(repeat, dim=0)
        return RecomputeDecoder(model, pe, k, Lmax) if warp is None else GuidedRecompute(model, pe, k, Lmax, base_embeds=base_embeds, min_keep=min_keep, **warp)
    if warp is not None and base_embeds is not None:
        return GuidedDecoder(model, prop_embeds, k, Lmax, repeat=repeat, xkv=xkv, base_embeds=base_embeds, min_keep=min_keep, **warp)
    dec = CachedDecoder(model, prop_embeds, k, Lmax, repeat=repeat, xkv=xkv)
    if warp is not None:
        dec.carry_warp(_decoder_warp(k, min_keep, None, **warp))
    return dec


def _advance(dec, book: BeamBook, ids: torch.Tensor, t: int, *, t_dev: torch.Tensor | None = None, noise=None, pick=None,
             ids_out: torch.Tensor | None = None) -> torch.Tensor:
    """One position of the search: the tokens `ids` at position t of every beam row -> the tokens at position t + 1, with the book and the
    decoder's ancestry brought up to date -- by the one-launch beam step (book.fused) or by pick, BeamBook.update and reorder.
    t_dev (int32 [1], device; cached decoder): the position comes from device memory in every launch and t is ignored, so the call can
    be captured once and replayed.  noise: the seeded search's source (_GumbelNoise).  pick(logits [N, k, V], noise) -> (log-probs, ids)
    [N, k, k]: the candidates of the tensor-op form (None: the k most probable).  ids_out: static buffer that receives the result."""
    logits = dec.step(ids, t) if t_dev is None else dec.step(ids, t, t_dev=t_dev)
    noise = None if noise is None else noise(t, book.mol)
    if book.fused:
        anc, rowmap = dec.search_tables()
        return book.step_fused(logits, anc, t_ptr=t_dev, t_off=0 if t_dev is None else 1, ids_out=ids_out, rowmap=rowmap, noise=noise)
    logits = logits.view(book.N, book.k, -1).float()
    values, indices = _pick(torch.softmax(logits, dim=-1), book.k, False) if pick is None else pick(logits, noise)
    held = None if t_dev is None else t_dev.to(torch.int64) + 1          # tokens held by every live beam (host: book.t = t + 1)
    parent, tok = book.update(values, indices, held)
    dec.reorder(parent, t + 1 if held is None else held)
    ids = tok.reshape(-1)
    return ids if ids_out is None else ids_out.copy_(ids)


def _start(dec, table, prefix: torch.Tensor | None, pair_of_molecule, k: int, max_steps: int, *, kernel: bool, prefill: bool = True):
    """The start of a search on a fresh decoder whose molecules have k rows each: molecule n starts from prefix[pair_of_molecule[n]]
    (check_prefix's result, int64 [Npairs, P], P >= 2: `prefill`, or with prefill=False its stepping twin) or, prefix None, from [CLS]
    alone.  table (syntax_table's result): the search is constrained, and its SyntaxMask (kernel: SyntaxMask's) becomes the decoder's
    `premask` before the first logits are taken.  -> (the logits of the first free position per row [len(pair_of_molecule) * k, V] --
    the k rows of a molecule hold the same history, so they are equal -- and the mask or None)."""
    pom = torch.as_tensor(pair_of_molecule).to(torch.int64)
    mask = None
    if table is not None:
        mask = SyntaxMask(table, k, 1 if prefix is None else int(prefix.shape[1]), max_steps, dec.device, kernel=kernel)
        mask.start(prefix, pom, len(pom))
    dec.premask = mask
    if prefix is None:
        return dec.step(torch.full((len(pom) * k,), CLS_ID, dtype=torch.long, device=dec.device), 0), mask
    return dec.prefill(prefix, pom, by_steps=not prefill)[pom.repeat_interleave(k).to(dec.device)], mask


def _search(model, dec, N: int, *, k: int, max_steps: int, sync_every: int = 4, stochastic: bool = False, generator=None, graph: bool = False,
            compact: bool = True, seed: int | None = None, mol_base: int = 0, need: int | None = None, prefix: torch.Tensor | None = None,
            pair_of_molecule=None, prefill: bool = True, table=None):
    """beam_search_batched behind the decoder's construction (generate_with_property builds its decoders from one encoded PV).
    need: finals that end a molecule's search (BeamBook; None: k).  prefix, pair_of_molecule (None: one pair per molecule), prefill,
    table: `_start`'s; the decoder was built for Lmax = P + max_steps + 2."""
    last_run.clear()
    dev = dec.device
    pom = torch.arange(N) if pair_of_molecule is None else torch.as_tensor(pair_of_molecule).to(torch.int64)
    P = 1 if prefix is None else int(prefix.shape[1])
    Lmax = P + max_steps + 2
    seeded = bool(stochastic and seed is not None)
    # one launch per position for the beam bookkeeping (csrc/decode.hip::beam_step_kernel: k <= 8 beams, vocabulary <= 512, histories <= 256
    # tokens -- the tensor-op bookkeeping serves everything else); spmm_gumbel_noise and spmm_smiles_mask accept the same shapes
    fits = bool(dec.cached and k <= 8 and model.cfg.text.vocab_size <= 512 and Lmax <= DECODE_MAXL)
    fused = bool(fits and FUSED_BEAM_STEP and (seeded or not stochastic))
    logits, mask = _start(dec, table, prefix, pom, k, max_steps, kernel=fused, prefill=prefill)
    logits = logits.view(N, k, -1)[:, 0].float()         # [N, V]: beam 0's
    V = logits.shape[-1]
    book = BeamBook(N, k, max_steps, dev, fused=fused, need=need, prefix=None if prefix is None else prefix[pom])
    noise_at = _GumbelNoise(seed, GUMBEL_SALT, mol_base + torch.arange(N), k, V, Lmax, dev, on_device=fits) if seeded else None

    def pick(logits, noise):
        if stochastic and not seeded and mask is not None:
            # torch.multinomial cannot draw k tokens from fewer than k non-zero probabilities; Gumbel-top-k from the generator's uniforms is
            # the same distribution and ranks the masked tokens last
            u = torch.rand(logits.shape, generator=generator, device=logits.device if generator is None else generator.device)
            return _pick_seeded(logits, -torch.log(-torch.log(u.clamp(1e-12, 1 - 1e-7))).to(logits.device), k)
        return _pick_seeded(logits, noise, k) if seeded else _pick(torch.softmax(logits, dim=-1), k, stochastic, generator)

    values, indices = pick(logits, noise_at(P - 1).view(N, k, -1)[:, 0] if seeded else None)      # (noise keyed by the absolute position)
    book.first(values, indices)
    ids = indices.reshape(N * k)
    if mask is not None:
        mask.book = book                                 # from here on the histories are the book's
    if graph and dec.cached and not stochastic and prefix is None and dec.warp is None and dec.premask is None:
        return _decode_graphed(dec, book, ids, max_steps, sync_every)
    n_cur = N
    last_run.update(molecules=N, compactions=0, final_batch=N, positions=0, prefix_tokens=P, prefill=bool(prefix is not None and prefill),
                    **dec.warp_info, syntax=mask is not None, dropped_masked=0)
    for s in range(max_steps):
        ids = _advance(dec, book, ids, P + s, noise=noise_at, pick=pick)
        last_run["positions"] = s + 1
        if s % sync_every != sync_every - 1:
            continue
        if not book.fused:
            if book.all_done():
                break
            continue
        n_live = N - int(book.n_done.item())         # the one host read of the loop
        if n_live == 0:
            break
        # molecules that hold their k finals stop costing anything: once a quarter of the batch is done the rest is gathered into
        # a smaller batch (caches stay where they are, CachedDecoder.compact)
        if compact and n_live <= COMPACT_BELOW * n_cur and n_cur - n_live >= 4:
            keep = book.live_slots()
            dec.compact(keep)
            book.compact(keep)
            ids = ids.view(n_cur, k)[keep].reshape(-1).contiguous()
            n_cur = int(keep.numel())
            last_run["compactions"] += 1
            last_run["final_batch"] = n_cur
    res = book.results()
    if mask is not None:
        # a hypothesis that went through a masked token carries <= -1e30 in its score; one that continued a struck-out [SEP] candidate (a
        # molecule with fewer than k live candidates) holds [SEP] inside -- its history rejects, so every token after it was masked alike
        kept = [[h for h in finals if h[0] > SYNTAX_DROP_BELOW and SEP_ID not in h[1][1:-1]] for finals in res]
        last_run["dropped_masked"] = sum(len(a) - len(b) for a, b in zip(res, kept))
        res = kept
    return res


def _decode_graphed(dec, book: BeamBook, ids: torch.Tensor, max_steps: int, sync_every: int):
    """The loop of beam_search_batched with every step-dependent scalar in device memory: two eager positions (they also set the
    kernels' one-time attributes), then one captured position replayed for the rest."""
    ids_s = ids.to(torch.int32).clone() if book.fused else ids.clone()      # static: the position's output is the next position's input
    t_dev = torch.ones(1, dtype=torch.int32, device=ids.device)  # position of the token in ids_s

    def one_position():
        _advance(dec, book, ids_s, 0, t_dev=t_dev, ids_out=ids_s)
        t_dev.add_(1)

    eager = min(2, max_steps)
    for _ in range(eager):
        one_position()
    steps_left = max_steps - eager
    if steps_left > 0 and not book.all_done():
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):      # other threads' GPU work does not abort this capture
            one_position()
        g.replay()                                               # capture records, it does not execute: this is position `eager`
        for s in range(1, steps_left):
            if s % sync_every == 0 and book.all_done():
                break
            g.replay()
    book.t = int(t_dev.item()) + 1
    return book.results()


@torch.no_grad()
def generate_with_property(model, pv: torch.Tensor, n_sample: int, prop_mask: torch.Tensor | None = None, k: int = 2, stochastic: bool = True,
                           seed: int = 0, max_steps: int = 100, chunk: int | None = None, prefix=None, prefill: bool = True, guidance: float = 1.0,
                           temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, syntax=None) -> List[List[int]]:
    """`generate_with_property` of d_pv2smiles_single.py:54-111: n_sample molecules from ONE (normalised) property vector pv [53], with the
    properties of prop_mask ([53], 1 = unspecified) replaced by the mask token.  Returns one token-id list per sample ([CLS] ... [SEP]; empty
    when the search of that sample finished nothing -- counted in last_generate["no_final"]).
    The PV is encoded once, on one row; the cross-attention keys / values are projected once per fusion layer and copied for the samples of
    a chunk (`chunk` samples are decoded together; None: all of them).  Sample i is molecule i of the seeded search (beam_search_batched(seed=...,
    mol_base=...)), so the samples do not depend on the chunking.  As in the reference (:102-110) a stochastic run returns one of each sample's
    up-to-k finals, picked by random.Random(seed) on the host in sample order; a deterministic run returns the best final.
    prefix (token ids [P], see beam_search_batched): every sample starts with it.  It is ONE (PV, prefix) pair: each chunk runs it
    through the decoder once into cache row 0, which every beam row of every sample of the chunk reads (prefill=False: stepped through on
    every row).  The samples still do not depend on the chunking: the noise is keyed by the absolute position.
    last_generate["prefix_tokens"] = P (1 without a prefix).
    guidance, temperature, top_k, top_p: beam_search_batched's, with the same checks and defaults (all at their defaults: the run without
    them).  The guidance baseline is this PV with every property masked; it is encoded once, and its cross-attention keys | values are
    projected once per run next to the condition's (`xkv_once`) -- a chunk of n samples is 2 conditions x n molecules in one decoder.  The
    samples still do not depend on the chunking.  last_generate records the four and baseline_rows.
    syntax: beam_search_batched's -- every sample returned is a well-formed SMILES string (syntax only), whatever the chunking: the mask
    of a row is a function of the row's own history.  last_generate records `syntax` and `dropped_masked`."""
    warp = check_warp(guidance, temperature, top_k, top_p, k)
    cached = hasattr(model, "engine")
    prefix = check_prefix(prefix, 1, _vocab_size(model), max_steps)
    table = syntax_table(model, syntax, prefix, max_steps)
    P = 1 if prefix is None else prefix.shape[1]
    prop_embeds = encode_properties(model, pv.reshape(1, -1), None if prop_mask is None else prop_mask.reshape(1, -1))
    if cached:
        model.engine.train_mode = False
    chunk = n_sample if not chunk else min(int(chunk), n_sample)
    rng = random.Random(seed)
    out: List[List[int]] = []
    xkv, none, dropped = None, 0, 0
    base_embeds = _baseline_embeds(model, pv) if warp is not None and warp["guidance"] != 1.0 else None
    for base in range(0, n_sample, chunk):
        n = min(chunk, n_sample - base)
        dec = make_decoder(model, prop_embeds, k, P + max_steps + 2, cached, warp, base_embeds=base_embeds, repeat=n, xkv=xkv)
        xkv = dec.xkv_once                               # projected by the first chunk's decoder, taken by the later ones
        res = _search(model, dec, n, k=k, max_steps=max_steps, stochastic=stochastic, seed=seed if stochastic else None, mol_base=base,
                      prefix=prefix, pair_of_molecule=[0] * n, prefill=prefill, table=table)
        dropped += last_run.get("dropped_masked", 0)
        for finals in res:
            if not finals:
                none += 1
                out.append([])
            else:
                out.append(finals[rng.randrange(len(finals)) if stochastic else 0][1])
    last_generate.clear()
    last_generate.update(samples=n_sample, no_final=none, chunks=(n_sample + chunk - 1) // chunk, prefix_tokens=P,
                         **{f: last_run.get(f, v) for f, v in dict(NO_WARP, baseline_rows=0).items()}, syntax=table is not None,
                         dropped_masked=dropped)
    return out


# ------------------------------------------------------------------------------------------------------------------
# Distinct samples: stochastic beam search (Kool, van Hoof, Welling 2019) -- sequences sampled WITHOUT replacement
# ------------------------------------------------------------------------------------------------------------------
DISTINCT_SALT = 0x53425331      # call-site salt of the distinct search's noise ("SBS1")
DISTINCT_MAX = 1024             # samples per property vector (spmm_sbs_step's W)
SBS_ALLOWED_ABOVE = -1e29       # a logit at or below this (-inf, the syntax mask's -1e30) is no candidate (spmm_sbs_step)
last_distinct: dict = {}        # what the last sample_distinct did: groups, W, n_distinct, positions, finished, unfinished, empty (per group, over
#                                 the first n_distinct slots), dropped_masked, fused, prefix_tokens, temperature, top_k, top_p, syntax, min_gap (the
#                                 tensor-op form: the smallest gap between unequal neighbouring keys a decision hung on; None on the kernel)


class DistinctBook:
    """The state of stochastic beam search for G property vectors x W slots, double-buffered: per slot the log-probability `phi` of its
    hypothesis, its perturbed key `gum` (-inf: the slot is empty), `fin`, `len`, the token history and the K/V ancestry row.  A step reads
    the current buffers and writes the others, then they swap: `step_fused` is the one-launch form (ops.sbs_step; fp32 state), `update`
    the same step as tensor ops in float64 (any device; whole-prefix decoders, shapes the kernel refuses, FUSED_BEAM_STEP = False).
    The search starts with slot 0 at phi = 0, gum = 0 and every other slot empty: the first position is a step like any other.
    `mol` is None and `tokens` / `t` read as BeamBook's: a SyntaxMask takes this book as it takes that one."""
    FIELDS = ("phi", "gum", "fin", "len", "tokens", "anc")

    def __init__(self, G: int, W: int, max_steps: int, device, fused: bool = False, prefix: torch.Tensor | None = None, anc: torch.Tensor | None = None):
        """prefix (int [G, P], P >= 1, prefix[:, 0] = [CLS]): every hypothesis of group g starts from prefix[g].  anc: the decoder's ancestry
        table after a prefill (None: every row reads its own cache row everywhere)."""
        P = 1 if prefix is None else int(prefix.shape[1])
        self.G, self.W, self.P, self.Lmax, self.fused = G, W, P, P + max_steps + 2, bool(fused)
        ft, it = (torch.float32, torch.int32) if fused else (torch.float64, torch.long)
        L = self.Lmax

        def state():
            return dict(phi=torch.full((G, W), -float("inf"), dtype=ft, device=device), gum=torch.full((G, W), -float("inf"), dtype=ft, device=device),
                        fin=torch.zeros(G, W, dtype=torch.uint8, device=device), len=torch.zeros(G, W, dtype=it, device=device),
                        tokens=torch.zeros(G, W, L, dtype=it, device=device),
                        anc=torch.arange(G * W, dtype=torch.int32, device=device)[:, None].repeat(1, L).contiguous())

        self.cur, self.nxt = state(), state()
        c = self.cur
        c["phi"][:, 0] = 0.0
        c["gum"][:, 0] = 0.0
        if prefix is None:
            c["tokens"][:, :, 0] = CLS_ID
        else:
            c["tokens"][:, :, :P] = prefix.to(device).to(it)[:, None, :]
        c["len"][:] = P
        if anc is not None:
            c["anc"].copy_(anc.reshape(G * W, L))
        self.t = P                                        # tokens held by every live slot
        self.open = torch.full((G,), W, dtype=torch.int32, device=device)
        self.ws = None                                    # the kernel's scratch (ops.sbs_step sizes it)
        self.mol = None
        self.parent = None                                # update: the parents of the last step, int64 [G, W]
        self.min_gap = float("inf")                       # update: the smallest gap between two unequal neighbours among the W + 1 best keys so far

    tokens = property(lambda self: self.cur["tokens"].view(self.G * self.W, self.Lmax))
    anc = property(lambda self: self.cur["anc"])

    def step_fused(self, logits: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        """One position as one launch: logits, noise fp32 [G*W, V] -> the tokens to feed next, int32 [G*W] (0 for finished and empty slots)."""
        ids = ops.sbs_step(logits, noise, self, t=self.t)
        self.cur, self.nxt = self.nxt, self.cur
        self.t += 1
        return ids

    def update(self, logits: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        """`step_fused` as tensor ops in float64 (the rules of spmm_sbs_step, include/spmm_hip.h) -> the tokens to feed next, int64 [G*W]."""
        G, W, L, t = self.G, self.W, self.Lmax, self.t
        c, n = self.cur, self.nxt
        V = logits.shape[-1]
        NEG = -float("inf")
        l, nz = logits.double().reshape(G, W, V), noise.double().reshape(G, W, -1)[:, :, :V].to(logits.device)
        T, phi, fin = c["gum"].double(), c["phi"].double(), c["fin"].bool()
        used = T > NEG
        live, done = used & ~fin, used & fin
        ok = (l > SBS_ALLOWED_ABOVE) & live[:, :, None]
        neg = torch.full_like(l, NEG)
        m = torch.where(ok, l, neg).max(-1, keepdim=True).values
        m0 = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        lse = m0 + torch.log(torch.where(ok, torch.exp(l - m0), torch.zeros_like(l)).sum(-1, keepdim=True))
        cphi = phi[:, :, None] + (l - lse)
        g = torch.where(ok, cphi + nz, neg)
        Z = g.max(-1, keepdim=True).values
        v = T[:, :, None] - g + torch.log1p(-torch.exp(g - Z))
        key = T[:, :, None] - v.clamp_min(0.0) - torch.log1p(torch.exp(-v.abs()))
        key = torch.where(ok & ~torch.isnan(key), key, neg)
        key[:, :, SEP_ID] = torch.where(done, T, key[:, :, SEP_ID])                 # a finished slot's one candidate: itself
        cphi[:, :, SEP_ID] = torch.where(done, phi, cphi[:, :, SEP_ID])
        skey, flat = torch.sort(key.reshape(G, W * V), dim=1, descending=True, stable=True)      # (stable: equal keys keep their flat-index order)
        top = skey[:, :W + 1]                            # the cut and the slot order hang on the gaps between these
        gaps = (top[:, :-1] - top[:, 1:])[(top[:, 1:] > NEG) & (top[:, :-1] > top[:, 1:])]
        if gaps.numel():
            self.min_gap = min(self.min_gap, float(gaps.min()))
        skey, flat = skey[:, :W], flat[:, :W]
        have = skey > NEG
        parent = torch.where(have, flat // V, torch.arange(W, device=flat.device)[None, :].expand(G, W))
        tok = torch.where(have, flat % V, torch.zeros_like(flat))
        pfin = fin.gather(1, parent) & have
        nfin = have & (pfin | (tok == SEP_ID))
        n["gum"] = torch.where(have, skey, torch.full_like(skey, NEG)).to(c["gum"].dtype)
        n["phi"] = torch.where(have, cphi.reshape(G, W * V).gather(1, flat), torch.full_like(skey, NEG)).to(c["phi"].dtype)
        n["fin"] = nfin.to(torch.uint8)
        n["len"] = torch.where(have, torch.where(pfin, c["len"].gather(1, parent), torch.full_like(c["len"], t + 1)), torch.zeros_like(c["len"]))
        tokens = c["tokens"].gather(1, parent[:, :, None].expand(G, W, L))
        tokens[:, :, t] = torch.where(pfin, tokens[:, :, t], tok.to(tokens.dtype))
        n["tokens"] = torch.where(have[:, :, None], tokens, torch.zeros_like(tokens))
        rows = torch.arange(G * W, device=flat.device).view(G, W)
        prow = (rows[:, :1] + parent).reshape(-1)
        own = rows.reshape(-1, 1).to(torch.int32).expand(G * W, L)
        inherit = (torch.arange(L, device=flat.device)[None, :] < t) & have.reshape(-1, 1)
        n["anc"] = torch.where(inherit, c["anc"][prow], own).contiguous()
        self.open = (have & ~nfin).sum(1).to(torch.int32)
        self.parent = parent
        self.cur, self.nxt = n, c
        self.t = t + 1
        return torch.where(have & ~nfin, tok, torch.zeros_like(tok)).reshape(-1)

    def results(self, n_first: int | None = None):
        """-> (per group the finished hypotheses among the first n_first slots, in slot order, as (logp, token ids); unfinished [G]; empty [G])."""
        n_first = self.W if n_first is None else n_first
        c = self.cur
        gum, phi, fin = c["gum"][:, :n_first].cpu(), c["phi"][:, :n_first].cpu(), c["fin"][:, :n_first].cpu().bool()
        ln, tk = c["len"][:, :n_first].cpu(), c["tokens"][:, :n_first].cpu()
        used = gum > -float("inf")
        out = [[(float(phi[g, s]), tk[g, s, : int(ln[g, s])].tolist()) for s in range(n_first) if used[g, s] and fin[g, s]] for g in range(self.G)]
        return out, (used & ~fin).sum(1).tolist(), (~used).sum(1).tolist()


@torch.no_grad()
def sample_distinct(model, props: torch.Tensor, n_distinct: int, prop_mask: torch.Tensor | None = None, seed: int = 0, max_steps: int = 100,
                    cached: bool | None = None, sync_every: int = 4, prefix=None, prefill: bool = True, temperature: float = 1.0, top_k: int = 0,
                    top_p: float = 1.0, syntax=None, guidance: float = 1.0, pv_base: int = 0) -> List[List[Tuple[float, List[int]]]]:
    """n_distinct DIFFERENT token sequences per property vector: stochastic beam search (Kool, van Hoof, Welling 2019), an exact sample
    without replacement from the model's sequence distribution.  props [53] or [G, 53]; result[g]: the finished hypotheses among the first
    n_distinct slots as (log-probability, token ids [CLS] .. [SEP]), in slot order -- sampling order, not probability order.  Hypotheses
    still open after max_steps positions are dropped and counted (last_distinct).
    The search runs W = n_distinct rounded up to a multiple of 8 slots and returns the first n_distinct: the noise of (seed, group,
    position, slot, token) does not depend on W (ops.gumbel_noise, k = 8, molecule (pv_base + g) * 128 + slot // 8), a slot's key never
    exceeds its parent's, and so the first n slots of a wider search ARE the n-slot search: one seed gives one ordered list of distinct
    sequences, and asking for more extends it.
    One launch per position for the bookkeeping where spmm_sbs_step takes the shape (cached decoder, vocabulary <= 512, <= 256 positions,
    FUSED_BEAM_STEP), the float64 tensor-op form elsewhere.  The decoder is the cached one (make_decoder: k = 8, repeat = W / 8) reading the book's current
    ancestry table (cached=False: the whole-prefix decoder); a finished slot's row keeps being stepped with token 0.  The search stays eager.
    prefix, prefill, syntax, temperature, top_k, top_p: beam_search_batched's, with min_keep = 1 (a row contributes any number of
    candidates); the log-probabilities returned are those of the warped distribution renormalised over the kept and allowed tokens.  A
    masked token is no candidate here, so no hypothesis goes through one.  guidance != 1 is not built: ValueError."""
    if float(guidance) != 1.0:
        raise ValueError(f"guidance={guidance}: classifier-free guidance is out of scope for sample_distinct (guidance = 1 only)")
    if isinstance(n_distinct, bool) or int(n_distinct) != n_distinct or not 1 <= int(n_distinct) <= DISTINCT_MAX:
        raise ValueError(f"n_distinct={n_distinct!r} outside [1, {DISTINCT_MAX}]: the search holds at most {DISTINCT_MAX} slots per property vector")
    n_distinct = int(n_distinct)
    warp = check_warp(1.0, temperature, top_k, top_p, 1)
    if cached is None:
        cached = hasattr(model, "engine")
    props = props.reshape(-1, props.shape[-1])
    G = props.shape[0]
    prefix = check_prefix(prefix, G, _vocab_size(model), max_steps)
    table = syntax_table(model, syntax, prefix, max_steps)
    P = 1 if prefix is None else prefix.shape[1]
    Lmax = check_positions(P + max_steps + 2, P)
    W = (n_distinct + 7) // 8 * 8
    k = 8 if cached else W                               # rows per decoder molecule: W / 8 molecules of 8 slots per group, or one of W
    prop_embeds = encode_properties(model, props, prop_mask)
    dev = prop_embeds.device
    if cached:
        model.engine.train_mode = False
    dec = make_decoder(model, prop_embeds, k, Lmax, cached, warp, repeat=W // k, min_keep=1)
    V = _vocab_size(model)
    fused = bool(cached and FUSED_BEAM_STEP and V is not None and 4 <= V <= 512)
    if prefix is not None:
        prefix = prefix.expand(G, P)
    # the (PV, prefix) pair of every decoder molecule is its group
    logits, mask = _start(dec, table, prefix, torch.arange(G * W // k) // (W // k), k, max_steps, kernel=fused, prefill=prefill)      # [G*W, V]
    V = logits.shape[-1]
    book = DistinctBook(G, W, max_steps, dev, fused=fused, prefix=prefix, anc=dec.anc if cached else None)
    # keyed by the absolute position of the last token held, as the seeded beam search keys its draws
    noise = _GumbelNoise(seed, DISTINCT_SALT, ((pv_base + torch.arange(G))[:, None] * 128 + torch.arange(W // 8)[None, :]).reshape(-1), 8, V, Lmax, dev,
                         on_device=fused)

    def advance(logits):
        ids = book.step_fused(logits.float(), noise(book.t - 1)) if fused else book.update(logits, noise(book.t - 1))
        if cached:
            dec.anc = book.anc                           # the decoder reads the book's current table; cache rows never move
        else:
            dec.reorder(book.parent, book.t - 1)
        return ids

    last_distinct.clear()
    ids = advance(logits)
    if mask is not None:
        mask.book = book
    positions = 0
    for s in range(max_steps):
        if s % sync_every == 0 and int(book.open.sum().item()) == 0:         # the one host read of the loop
            break
        ids = advance(dec.step(ids, P + s))
        positions = s + 1
    res, unfinished, empty = book.results(n_distinct)
    kept = [[h for h in hyps if h[0] > SYNTAX_DROP_BELOW] for hyps in res]
    last_distinct.update(groups=G, W=W, n_distinct=n_distinct, positions=positions, finished=[len(h) for h in kept], unfinished=unfinished, empty=empty,
                         dropped_masked=sum(len(a) - len(b) for a, b in zip(res, kept)), fused=fused, prefix_tokens=P,
                         min_gap=None if fused else book.min_gap,
                         **{f: (warp or NO_WARP)[f] for f in ("temperature", "top_k", "top_p")}, syntax=mask is not None)
    return kept


# ------------------------------------------------------------------------------------------------------------------
# SMILES -> PV: 53 autoregressive regression steps
# ------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def smiles_to_pv(model, text_ids: torch.Tensor, text_mask: torch.Tensor, n_props: int = 53) -> torch.Tensor:
    """Predict the (normalised) property vector of every SMILES in the batch, one property per step, as
    d_smiles2pv.py:14-52 does: the text is encoded once by the unimodal text layers; at step i the PV prefix
    [CLS, p_0..p_{i-1}] goes through the (bidirectional) PV encoder, then causally through the fusion layers with
    cross-attention to the text, and `property_mtr_head` reads property i off the last position.  The whole batch advances
    together; the prefix is re-encoded every step because the PV encoder is bidirectional (nothing to cache).
    text_ids / text_mask: [B, Lt] without the tokenizer's own [CLS] (the caller drops column 0, SPMM_models.py:357).
    Returns [B, n_props] in the normalised space (de-normalise with the dataset's mean/std as d_smiles2pv.py:49 does)."""
    text_embeds = model.text_encoder.bert(text_ids, attention_mask=text_mask, return_dict=True, mode="text").last_hidden_state
    B, dev = text_embeds.shape[0], text_embeds.device
    cls = model.property_cls
    prefix = cls.detach().to(dev).to(text_embeds.dtype).expand(B, -1, -1)
    out = []
    for _ in range(n_props):
        pv = model.property_encoder(inputs_embeds=prefix, return_dict=True).last_hidden_state
        ones = torch.ones(pv.shape[:-1], dtype=torch.long, device=dev)
        fused = model.text_encoder.bert(encoder_embeds=pv, attention_mask=ones, encoder_hidden_states=text_embeds,
                                        encoder_attention_mask=text_mask.to(dev), return_dict=True, is_decoder=True,
                                        mode="fusion").last_hidden_state
        nxt = model.property_mtr_head(fused[:, -1:, :]).reshape(B)            # only the last position is read (:25)
        out.append(nxt)
        prefix = torch.cat([prefix, model.property_embed(nxt.reshape(B, 1, 1)).to(prefix.dtype)], dim=1)
    return torch.stack(out, dim=-1)


class S2PDecoder:
    """`smiles_to_pv` on the engine.  What does not change between the steps is computed once: the text is encoded once on packed rows
    (padding rows dropped, as the fine-tuning step packs them), the cross-attention keys | values of every fusion layer are projected
    once from it, and the embedded prefix rows live in an append-only cache `xcache` [B, n_props + 1, H] -- the embedded row of prefix
    position j depends on the value at j and on j alone.  The PV encoder is bidirectional, so every hidden state of the prefix changes
    at every step: nothing else can be cached.  A step is launches only -- the row count B * n is host data -- and its last fusion
    layer runs on the B last-position rows, the only ones read afterwards, with self-attention keys / values projected from all B * n
    rows (engine.SelfKV).  `pred` [B, n_props] fp32 fills one column per step (ops.s2p_append)."""
    TP = "text_encoder.bert."

    @torch.no_grad()
    def __init__(self, model, text_ids: torch.Tensor, text_mask: torch.Tensor, n_props: int = 53, n_tokens: Optional[int] = None):
        from .engine import BF, host_token_count
        eng = model.engine
        eng.train_mode = False
        self.eng, self.P, self.ct, self.cp = eng, eng.P, model.cfg.text, model.cfg.prop
        ct, cp, P, dev = self.ct, self.cp, eng.P, model.device_
        H = ct.hidden_size
        B = text_ids.shape[0]
        Lc = n_props + 1
        if Lc > cp.max_position_embeddings:
            raise ValueError(f"{n_props} properties need {Lc} positions; the PV encoder has {cp.max_position_embeddings}")
        self.B, self.n_props, self.Lc, self.H = B, n_props, Lc, H
        # ---- the text, once: embeddings, packed rows, unimodal layers
        text = eng.encode_text(self.TP, ct, text_ids.to(dev).to(torch.int32).contiguous(), text_mask.to(dev).to(torch.int32).contiguous(),
                               n_tokens=host_token_count(text_mask) if n_tokens is None else int(n_tokens))      # (given: a device mask)
        # ---- cross-attention keys | values of every fusion layer, once
        proj = {f"{self.TP}encoder.layer.{l}.crossattention": KV for l, KV in _cross_kv(eng, self.TP, ct, text.y).items()}
        self.src = text.source(proj=proj)
        self.kv_mask = text.kv_mask                      # (packed: the source's lengths are the key mask)
        self.ar = torch.arange(B, dtype=torch.int32, device=dev)
        # ---- index arrays of all steps, once: step i gathers rows (b, 0..i) of the cache and keeps row (b, i) for the last layer
        b_ = np.arange(B, dtype=np.int64)[:, None]
        gather = [(b_ * Lc + np.arange(i + 1, dtype=np.int64)[None, :]).reshape(-1) for i in range(n_props)]
        self.off = np.concatenate([[0], np.cumsum([a.size for a in gather])])
        self.idx = torch.from_numpy(np.concatenate(gather)).to(dev)
        steps = np.arange(1, n_props + 1, dtype=np.int64)[:, None]
        self.last = torch.from_numpy(np.ascontiguousarray(b_.T * steps + steps - 1)).to(dev)                 # int64 [n_props, B]
        self.row0 = torch.from_numpy(np.ascontiguousarray((b_.T * steps).astype(np.int32))).to(dev)         # int32 [n_props, B]
        self.lens = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(steps, (n_props, B)).astype(np.int32))).to(dev)
        # ---- the cache: row 0 of every molecule is the embedded property_cls (BertEmbeddings, inputs_embeds branch)
        self.xcache = torch.empty(B, Lc, H, dtype=BF, device=dev)
        cls = P.w("property_cls").reshape(1, H).expand(B, H).contiguous()
        self.xcache[:, 0] = eng.embed_generic("property_encoder.", cp, cls, B, 1)
        self.pred = torch.empty(B, n_props, dtype=torch.float32, device=dev)
        ep = "property_encoder.embeddings."
        self.emb = dict(pe_w=P.w("property_embed.weight").reshape(H), pe_b=P.w("property_embed.bias"), pos=P.w(ep + "position_embeddings.weight"),
                        type0=P.w(ep + "token_type_embeddings.weight")[0], gamma=P.w(ep + "LayerNorm.weight"), beta=P.w(ep + "LayerNorm.bias"),
                        eps=cp.layer_norm_eps)

    @torch.no_grad()
    def step(self, i: int):
        """Property i of every molecule from the prefix [CLS, p_0 .. p_{i-1}] held by the cache -> pred[:, i]; appends prefix row i + 1."""
        from .engine import Batch, Group, SelfKV
        eng, P, ct, cp, B, H = self.eng, self.P, self.ct, self.cp, self.B, self.H
        n, f, nl = i + 1, ct.fusion_layer, ct.num_hidden_layers
        x = ops.gather_rows(eng._new(B * n, H), self.xcache.view(B * self.Lc, H), self.idx[self.off[i]:self.off[i + 1]])
        pv, _, _ = eng.stack_fwd("property_encoder.", cp, range(cp.num_hidden_layers), False, x, Batch([Group(0, B, n, None, B)]), False)
        g_lo = Batch([Group(0, B, n, None, 0, kv_mask=self.kv_mask).bind(self.src, self.ar, 0)])
        y, _, _ = eng.stack_fwd(self.TP, ct, range(f, nl - 1), True, pv, g_lo, False)
        # the last fusion layer on the B last-position rows (a causal query at position n - 1 sees every key of its sequence)
        xt = ops.gather_rows(eng._new(B, H), y, self.last[i])
        g_top = Batch([Group(0, B, 1, None, B, kv_mask=self.kv_mask, self_src=SelfKV(y), skv_row0=self.row0[i], skv_len=self.lens[i],
                             skv_L=n).bind(self.src, self.ar, 0)])
        yt, _, _ = eng._layer_fwd(f"{self.TP}encoder.layer.{nl - 1}.", ct, True, xt, g_top, False)
        h, _ = eng._transform_fwd("property_mtr_head.0", "property_mtr_head.2", yt, False, eps=ct.layer_norm_eps, pre=False)
        ops.s2p_append(h, P.w("property_mtr_head.3.weight").reshape(H), P.w("property_mtr_head.3.bias"), self.pred, i, n_props=self.n_props,
                       xcache=self.xcache, **self.emb)


@torch.no_grad()
def predict_properties(model, text_ids: torch.Tensor, text_mask: torch.Tensor, n_props: int = 53, n_tokens: Optional[int] = None) -> torch.Tensor:
    """`smiles_to_pv` (same arguments, same [B, n_props] normalised result) on the engine: S2PDecoder.  A model without an engine -- the
    CPU oracle, any foreign module exposing the reference's sub-module API -- goes through `smiles_to_pv` itself.  n_tokens: the host's
    count of valid tokens when the mask lives on the device (it sizes the packed text rows without a device read)."""
    if not hasattr(model, "engine"):
        return smiles_to_pv(model, text_ids, text_mask, n_props)
    dec = S2PDecoder(model, text_ids, text_mask, n_props, n_tokens=n_tokens)
    for i in range(n_props):
        dec.step(i)
    return dec.pred


# ------------------------------------------------------------------------------------------------------------------
# Reaction prediction (d_rxn_prediction.py, SPMM_models_rxn.py): the decoder cross-attends to the encoded reactant SMILES
# ------------------------------------------------------------------------------------------------------------------
RXN_MAX_STEPS = 100             # positions of `evaluate` / `evaluate_beam` (d_rxn_prediction.py:67,100)


class RxnDecoder(CachedDecoder):
    """The cached decoder of reaction prediction: the cross-attention memory of reaction n is its encoded reactant SMILES, 1 .. 256 tokens,
    different for every reaction of the batch.  The reactants are encoded once by `text_encoder2` on packed rows (padding rows dropped, as
    S2PDecoder encodes its text), the keys | values of every fusion layer are projected once from those rows, and the packed rows' start /
    length tables are what spmm_decode_xattn reads them through.  text_mask: right-padded prefixes with at least one token each."""
    EP = "text_encoder2.bert."

    @torch.no_grad()
    def __init__(self, model, text_ids: torch.Tensor, text_mask: torch.Tensor, k: int, Lmax: int):
        from .engine import host_token_count
        eng, ce, dev = model.engine, model.cfg_enc, model.device_
        eng.train_mode = False
        B, Lt = text_ids.shape
        if not 1 <= k <= 8:
            raise ValueError(f"{k} beams: spmm_decode_xattn serves 1..8 beams per reaction")
        if Lt > ops.ATTN_MAXL:
            raise ValueError(f"reactant sequences are limited to {ops.ATTN_MAXL} tokens (got {Lt}); the reference truncates at 150")
        host_mask = text_mask.detach().to("cpu")
        n_tokens = host_token_count(host_mask)
        if tuple(host_mask.shape) != (B, Lt) or n_tokens is None:
            raise ValueError("text_mask must be [B, Lt] right-padded prefixes with at least one token per reaction")
        text = eng.encode_text(self.EP, ce, text_ids.to(dev).to(torch.int32).contiguous(), host_mask.to(dev).to(torch.int32).contiguous(),
                               n_tokens=n_tokens)                                                        # mode='text'
        row0, length = text.tables()                     # (nothing to drop, or packing switched off: those of the dense [B, Lt] rows)
        memory = dict(N=B, Lmax=Lt, xkv=_cross_kv(eng, "text_encoder.bert.", model.cfg.text, text.y), row0=row0.contiguous(), len=length.contiguous())
        super().__init__(model, None, k, Lmax, memory=memory)
        self.src_len = host_mask.sum(1).to(torch.int32)  # host: tokens per reaction


class _HostBeams:
    """`evaluate_beam` (d_rxn_prediction.py:86-123) for one reaction through `model.generate`: whole-prefix forwards, host bookkeeping."""

    def __init__(self, model, embeds, mask, k):
        self.model, self.embeds, self.mask, self.k = model, embeds, mask, k

    def top(self, prefix):
        lp, ids = self.model.generate(self.embeds, self.mask, prefix, stochastic=False, k=self.k)
        return lp.float(), ids

    def run(self, max_steps):
        k, dev = self.k, self.embeds.device
        cls = torch.full((1, 1), CLS_ID, dtype=torch.long, device=dev)
        lp, ids = self.top(cls)
        beams = torch.cat([cls.expand(k, 1), ids.reshape(k, 1)], dim=1)
        score = lp.reshape(k)
        finals = []
        for _ in range(max_steps):
            lp, ids = self.top(beams)
            cand_p = score[:, None] + lp
            cand = torch.cat([beams[:, None, :].expand(k, k, beams.shape[1]), ids[:, :, None]], dim=2)
            hits = (ids == SEP_ID).nonzero(as_tuple=False).tolist()                 # row-major
            for b, j in hits:
                finals.append((float(cand_p[b, j]), cand[b, j].tolist()))
                cand_p[b, j] = -1e5
            if hits and len(finals) >= k * k:
                break
            score, flat = torch.topk(cand_p.reshape(-1), k)
            beams = cand.reshape(k * k, -1)[flat]
        finals.sort(key=lambda h: h[0], reverse=True)                               # (stable)
        return finals[:k]


def _encode_reactants(model, text_ids, text_mask):
    return model.text_encoder2.bert(text_ids, attention_mask=text_mask, return_dict=True, mode="text").last_hidden_state


@torch.no_grad()
def predict_products(model, text_ids: torch.Tensor, text_mask: torch.Tensor, k: int = 5, max_steps: int = RXN_MAX_STEPS, cached: bool | None = None,
                     sync_every: int = 4, compact: bool = True) -> List[List[Tuple[float, List[int]]]]:
    """`evaluate_beam` of d_rxn_prediction.py for a batch of reactions: text_ids / text_mask [N, Lt] are the reactant tokens as the encoder
    sees them ([CLS] pieces [SEP] PAD.., the tokenizer's own first token dropped).  result[n]: up to k (log-prob, ids incl. [CLS] and [SEP]),
    best first -- the k best of the k*k hypotheses the search collects before it stops (or of those that ended within max_steps positions).
    cached=True (default on the HIP model): all reactions together on the engine (RxnDecoder, the one-launch beam step when it takes the
    shape), finished reactions dropped as the search goes (`compact`).  cached=False: the reference's loop, one reaction at a time through
    `model.text_encoder2.bert` and `model.generate` -- every position re-runs the whole prefix and re-projects the memory; it runs on any
    object with that API."""
    if cached is None:
        cached = hasattr(model, "engine")
    N = text_ids.shape[0]
    if cached:
        dec = RxnDecoder(model, text_ids, text_mask, k, max_steps + 3)
        return _search(model, dec, N, k=k, max_steps=max_steps, sync_every=sync_every, compact=compact, need=k * k)
    out = []
    for n in range(N):
        L = max(int(text_mask[n].sum()), 1)
        ids, mask = text_ids[n:n + 1, :L], text_mask[n:n + 1, :L]
        out.append(_HostBeams(model, _encode_reactants(model, ids, mask), mask, k).run(max_steps))
    return out


@torch.no_grad()
def greedy_products(model, text_ids: torch.Tensor, text_mask: torch.Tensor, max_steps: int = RXN_MAX_STEPS, cached: bool | None = None,
                    sync_every: int = 4) -> List[List[int]]:
    """`evaluate` of d_rxn_prediction.py:56-81: the most probable next token of every reaction for up to max_steps positions, stopped once
    every reaction has produced [SEP].  result[n]: the ids from [CLS] up to and including the first [SEP], or all max_steps + 1 of them when
    there is none.  cached=True: one beam per reaction on the engine, ended flags on the device, one host read every `sync_every`
    positions.  cached=False: the whole batch through `model.generate`, the prefix re-run at every position."""
    if cached is None:
        cached = hasattr(model, "engine")
    N = text_ids.shape[0]
    if cached:
        dec = RxnDecoder(model, text_ids, text_mask, 1, max_steps + 3)
        dev = dec.device
        toks = torch.zeros(N, max_steps + 1, dtype=torch.long, device=dev)
        toks[:, 0] = CLS_ID
        ended = torch.zeros(N, dtype=torch.bool, device=dev)
        ids = toks[:, 0].contiguous()
        last_run.clear()
        last_run.update(molecules=N, compactions=0, final_batch=N, positions=0)
        for t in range(max_steps):
            ids = torch.argmax(dec.step(ids, t), dim=-1)
            toks[:, t + 1] = ids
            ended |= ids == SEP_ID
            last_run["positions"] = t + 1
            if t % sync_every == sync_every - 1 and bool(ended.all()):
                break
        toks = toks.cpu()
    else:
        embeds = _encode_reactants(model, text_ids, text_mask)
        toks = torch.full((N, 1), CLS_ID, dtype=torch.long, device=embeds.device)
        ended = torch.zeros(N, 1, dtype=torch.bool, device=embeds.device)
        for _ in range(max_steps):
            nxt = model.generate(embeds, text_mask, toks, stochastic=False)
            ended |= nxt == SEP_ID
            toks = torch.cat([toks, nxt], dim=-1)
            if bool(ended.all()):
                break
        toks = toks.cpu()
    out = []
    for row in toks.tolist():
        row = row[:max_steps + 1]
        out.append(row[:row.index(SEP_ID) + 1] if SEP_ID in row else row)
    return out
