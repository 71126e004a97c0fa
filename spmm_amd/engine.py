"""Step engine: schedules the HIP kernels of one SPMM pretraining step (forward, backward) on the current stream.

The twelve encoder passes of SPMM.forward (SPMM_models.py:79-256, table in SURVEY.md section 3.1) are merged into six
token-major batches that share weights, so every GEMM sees a large M and weights are streamed once per layer:

  S1  PV student      layers 0..n   : P1 | P11(causal)                        2B x 54 tokens
  S2  text student    layers 0..f-1 : P2 | P10a(causal)                       2B x Lt
  S3  PV momentum                   : P3                                       B x 54          (no grad)
  S4  text momentum   layers 0..f-1 : P4 | P9a(causal)                        2B x Lt          (no grad)
  S5  text momentum   layers f..n-1 : P9b(causal, cross -> prop_embeds_m) + LM head            (no grad)
  S6  text student    layers f..n-1 : [P5 | P7 | P12(causal)] query-PV rows (4B x 54) ++
                                      [P6 | P8 | P10b(causal)] query-text rows (4B x Lt), cross-attending each other

Three exact work reductions sit on top (spmm_amd/step.py): cross-attention K/V projected once per unique source sequence
(KVSource), padding-token rows dropped from the passes whose losses read only position 0 (packed layouts), and the
independent chains S1 | S2 | S4 (and S5 under S6) on separate HIP streams.

There is no autograd inside: forward keeps an explicit tape of the activations backward needs, backward walks it.
Everything that changes between steps (alpha, lr, dropout seed, loss-gradient scales, queue pointer) is read from
device memory; the one host read per step is the packed row count that sizes the GEMMs (PretrainStep._pack_plan)."""
from __future__ import annotations

import contextlib
import functools
from dataclasses import dataclass
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import ops, streams
from .config import BertConfig, SPMMConfig
from .options import EngineOptions
from .params import ParamStore

BF = torch.bfloat16
LOSS_MLM, LOSS_MPM, LOSS_ITA, LOSS_ITM = 0, 1, 2, 3


def _ceil(x, m):
    return (x + m - 1) // m * m


class KVSource:
    """Key/value source of a cross-attention shared by several query sequences (possibly of several groups): `kv` holds U
    unique sequences of up to Lkv tokens -- dense ([U*Lkv, H]) or packed (row0/len int32 [U], `pack_idx` = dense row of every
    packed row).  Each consumer group registers its sequence -> source map; K/V are projected once per layer, and in backward
    the consumers' dK/dV are folded onto the unique rows (CSR inverse map) before the weight- and data-gradient GEMMs."""

    def __init__(self, kv: torch.Tensor, U: int, Lkv: int, row0=None, length=None, pack_idx=None, proj=None):
        self.kv, self.U, self.Lkv, self.row0, self.len, self.pack_idx = kv, U, Lkv, row0, length, pack_idx
        # inference over many passes against ONE source (decode.S2PDecoder): {cross-attention prefix: projected keys | values [rows, 2H]},
        # projected once by the caller; a block whose prefix is listed reads them instead of projecting `kv` again
        self.proj = proj
        self._idx: List[torch.Tensor] = []
        self.nseq = 0
        self.start = self.list = None

    def add(self, idx: torch.Tensor) -> int:
        """Registers consumer sequences (idx int64 [n]: source of each); returns their offset in the consumer numbering."""
        off = self.nseq
        self._idx.append(idx)
        self.nseq += idx.numel()
        return off

    def preset(self, nseq: int, start: torch.Tensor, lst: torch.Tensor):
        """The inverse map computed elsewhere (csrc/plan.hip::fusion_plan_kernel) instead of finalize(); consumers then `bind`."""
        self.nseq, self.start, self.list = nseq, start, lst
        return self

    def finalize(self):
        idx = torch.cat(self._idx)
        order = torch.sort(idx, stable=True).indices
        start = torch.zeros(self.U + 1, dtype=torch.int32, device=idx.device)
        counts = torch.zeros(self.U, dtype=torch.int64, device=idx.device).index_add_(0, idx, torch.ones_like(idx))
        start[1:] = torch.cumsum(counts, 0)             # (torch.bincount reads max(idx) back to the host: a hidden sync per source)
        self.start, self.list = start, order.to(torch.int32)
        return self


@dataclass
class SelfKV:
    """Private SELF-attention key/value source of groups that keep only some query rows of their sequences (the CLS-only top fusion
    layer, step.py): keys / values are projected from `x` -- rows of the layer input, every token of the sequences -- with the layer's own
    key / value weights; a group's sequence s owns skv_len[s] rows from row skv_row0[s] of x.  Backward writes d(loss)/dx into `dx`."""
    x: torch.Tensor
    dx: Optional[torch.Tensor] = None
    rows_dev: Optional[torch.Tensor] = None      # device-side row count of x (int32 [1]) when only the device knows it


@dataclass
class Group:
    """A run of `nseq` sequences inside a token-major batch, attended independently: dense (`L` rows each) or packed
    (`q_len[s]` rows from row `q_row0[s]`, relative to row0; `nrows` rows in total)."""
    row0: int
    nseq: int
    L: int
    kmask: Optional[torch.Tensor]          # int32 [nseq, L] (1 = attend) or None
    causal_from: int                       # sequences >= causal_from (within the group) are causal
    kv: Optional[torch.Tensor] = None      # private cross-attention source, bf16 [nseq*Lkv, H] (facades, momentum pass)
    Lkv: int = 0
    kv_mask: Optional[torch.Tensor] = None
    q_row0: Optional[torch.Tensor] = None  # int32 [nseq]
    q_len: Optional[torch.Tensor] = None   # int32 [nseq]
    nrows: int = -1
    src: Optional[KVSource] = None         # shared cross-attention source ...
    kv_idx: Optional[torch.Tensor] = None  # ... int32 [nseq]: the source sequence each query sequence attends
    kv_off: int = 0                        # ... offset of this group's sequences in the source's consumer numbering
    self_src: Optional[SelfKV] = None      # self-attention keys / values from the full sequences (query rows are a subset) ...
    skv_row0: Optional[torch.Tensor] = None    # ... int32 [nseq]: first row of sequence s in self_src.x
    skv_len: Optional[torch.Tensor] = None     # ... int32 [nseq]
    skv_L: int = 0                             # ... longest sequence

    @property
    def rows(self):
        n = self.nrows if self.nrows >= 0 else self.nseq * self.L
        return slice(self.row0, self.row0 + n)

    def bind(self, src: KVSource, kv_idx: torch.Tensor, kv_off: int) -> "Group":
        """attend() for a source whose consumer numbering is preset: kv_idx int32 [nseq], kv_off = this group's offset in it."""
        self.src, self.Lkv, self.kv_idx, self.kv_off = src, src.Lkv, kv_idx, kv_off
        return self

    def attend(self, src: KVSource, idx: torch.Tensor) -> "Group":
        self.src, self.Lkv = src, src.Lkv
        self.kv_off = src.add(idx)
        self.kv_idx = idx.to(torch.int32)
        return self

    def cross_layout(self) -> dict:
        """Layout arguments of this group's cross-attention launches (forward, backward, fused form)."""
        src = self.src
        return dict(kmask=self.kv_mask, kv_seq=self.kv_idx, q_row0=self.q_row0, q_len=self.q_len,
                    kv_row0=None if src is None else src.row0, kv_len=None if src is None else src.len)


@dataclass
class Batch:
    """A token-major batch as the layers see it: its groups and -- when only the device knows it -- its row count.  The fusion batch of
    the packed path ends with the text hard negatives drawn on the device: their total length, and so the batch's row count, is device
    data; the batch is allocated for the most it can be and every launch over ITS rows takes the real count from `rows_dev` ("device-side
    row counts" in include/spmm_hip.h).  Launches over other row sets (key/value sources, SelfKV) never do."""
    groups: List[Group]
    rows_dev: Optional[torch.Tensor] = None      # int32 [1] on the device; None: the host-side row count is exact

    def __iter__(self):
        return iter(self.groups)

    def __len__(self):
        return len(self.groups)


@dataclass
class LnTape:
    """What the backward of one LayerNorm needs, whichever forward ran it (composite or fused residual sublayer, embeddings, transform heads):
    the pre-norm sum z (None: the normalised values come from the output y, EngineOptions.ln_from_y), row statistics, dropout salt."""
    z: Optional[torch.Tensor]
    y: Optional[torch.Tensor]
    mean: Optional[torch.Tensor]
    rstd: Optional[torch.Tensor]
    salt: int = 0


@dataclass
class HeadTape:
    """Engine._transform_fwd: parameter names of the dense layer and the LayerNorm, input, GELU pre-activation, the LayerNorm's record."""
    dense: str
    norm: str
    X: torch.Tensor
    pre: Optional[torch.Tensor]
    ln: LnTape


def _prefix_lens(mask_h: torch.Tensor) -> Optional[torch.Tensor]:
    """Row sums of a host mask [n, L]; None unless every row is a non-empty prefix."""
    lens = mask_h.sum(1)
    prefix = bool((lens > 0).all()) and bool(((torch.arange(mask_h.shape[1])[None, :] < lens[:, None]) == (mask_h != 0)).all())
    return lens if prefix else None


def host_lens(mask_h: torch.Tensor, what: str) -> np.ndarray:
    """Token counts of a host mask [n, L] whose rows are non-empty prefixes (what padding a batch to its longest gives)."""
    if mask_h.dim() != 2 or mask_h.shape[0] == 0:
        raise ValueError(f"{what}: the attention mask must be [n, L] with n >= 1")
    lens = _prefix_lens(mask_h)
    if lens is None:
        raise ValueError(f"{what}: every attention mask must be a non-empty prefix (what padding a batch to its longest gives)")
    return lens.numpy().astype(np.int64)


def host_token_count(mask) -> Optional[int]:
    """Valid-token count of a host mask whose rows are non-empty prefixes (what padding='longest' gives): sizes the packed layers
    (Engine._pack_plan's `n_tokens`) without a device read.  None for a device mask or another shape of mask (the pack plan then reads
    the count back itself)."""
    if not (torch.is_tensor(mask) and mask.device.type == "cpu" and mask.dim() == 2):
        return None
    lens = _prefix_lens(mask)
    return None if lens is None else int(lens.sum())


class PairLayout(NamedTuple):
    """P query sequences gathered from U distinct sequences of a text pass (TextRows.pair_layout), host arrays: pair p is `len_p[p]` rows
    from row `qrow0[p]` of the Mt gathered rows; gathered row r is position `pos[r]` of pair `seq[r]` = row `gather[r]` of the pass."""
    len_p: np.ndarray
    qrow0: np.ndarray
    Mt: int
    pos: np.ndarray
    seq: np.ndarray
    gather: np.ndarray


@dataclass
class TextRows:
    """One batch of token ids as the text layers take it (Engine.text_rows_of) and, after Engine.encode_text, what they made of it:
    the valid rows of the pack plan `pk`, or -- pk None -- the dense [B * L] rows under their key mask."""
    x: torch.Tensor                        # embedded rows, bf16 [M, H]
    groups: Batch                          # one Group of B sequences
    pk: Optional[dict]                     # the pack plan (ops.pack_plan), None: dense rows
    cls_rows: torch.Tensor                 # int64 [B]: the row of position 0 of every sequence
    ids32: torch.Tensor
    mask32: torch.Tensor
    B: int
    L: int
    esv: LnTape                            # the embedding's tape
    y: Optional[torch.Tensor] = None       # encode_text: the output of layers 0 .. fusion_layer - 1 ...
    tape: Optional[list] = None            # ... and their tape

    @property
    def kv_mask(self):
        """Key padding mask of a cross-attention over these rows: a packed source implies its key padding by its lengths."""
        return None if self.pk else self.mask32

    def tables(self):
        """-> (row0, len) int32 [B] on the device: first row and row count of every sequence, whichever layout the rows have."""
        if self.pk:
            return self.pk["row0"], self.pk["len"]
        return torch.arange(self.B, dtype=torch.int32, device=self.mask32.device) * self.L, self.mask32.sum(1).to(torch.int32)

    def source(self, proj=None, tables: bool = False) -> KVSource:
        """The encoded rows as a shared cross-attention source.  Dense rows carry no tables (their consumers pass `kv_mask`) unless
        `tables` asks for the dense ones: the attention kernels specialise on which of the two they are given."""
        row0, length = self.tables() if (self.pk or tables) else (None, None)
        return KVSource(self.y, self.B, self.L, row0=row0, length=length, pack_idx=self.pk["rows"] if self.pk else None, proj=proj)

    def pair_layout(self, lens_u: np.ndarray, inv: np.ndarray) -> PairLayout:
        """lens_u: the host's token counts of the B sequences; inv [P]: the sequence of every pair."""
        row0_u = np.concatenate([[0], np.cumsum(lens_u)[:-1]]) if self.pk else np.arange(self.B, dtype=np.int64) * self.L
        len_p = lens_u[inv]
        qrow0 = np.concatenate([[0], np.cumsum(len_p)[:-1]])
        pos = np.concatenate([np.arange(l) for l in len_p])
        seq = np.repeat(np.arange(len(inv)), len_p)
        return PairLayout(len_p, qrow0, int(len_p.sum()), pos, seq, row0_u[inv][seq] + pos)


STREAM_TOKENS_MAX = 49152         # B x Lt above which the step runs on one stream (Engine._one_stream)


class Engine:
    def __init__(self, cfg: SPMMConfig, params: ParamStore, device, options: Optional[EngineOptions] = None):
        self.cfg, self.P, self.dev = cfg, params, device
        self.opt = options if options is not None else EngineOptions.from_env()
        if torch.device(device).type == "cuda":
            from ._lib import bind_device
            bind_device(torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device())
        f32 = dict(dtype=torch.float32, device=device)
        self.alpha = torch.zeros(1, **f32)
        self.lr = torch.zeros(1, **f32)
        self.gscale = torch.ones(4, **f32)                 # d(total)/d(loss_k), order (mlm, mpm, ita, itm)
        # what every step starts from zero -- the four losses, d(ita)/d(temp), the non-finite flag, the token-hint flag -- is ONE 64-byte
        # buffer, zeroed by one launch at the head of the step (step.py)
        self.step_zero = torch.zeros(16, dtype=torch.int32, device=device)
        self.losses = self.step_zero[0:8].view(torch.float32)
        self.loss_scratch = torch.zeros(8, **f32)
        # dropout / negative-sampling seed: a device counter advanced once per training-mode forward (step.py), different on every
        # data-parallel rank, saved and restored with the checkpoint (model.py)
        rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
        self.seed_rank_offset = rank * 0x9E3779B97F4A7C15 % (1 << 62)      # (checkpoints hold the rank-independent part: model.py)
        self.seed = torch.full((1,), (0x5DEECE66D + self.seed_rank_offset) % (1 << 62), dtype=torch.int64, device=device)
        self.nan_flag = self.step_zero[9:10]
        self.icount = torch.zeros(8, dtype=torch.int32, device=device)      # two 4-int workspaces: lm_loss, mpm_head
        self.dtemp_ita = self.step_zero[8:9].view(torch.float32)
        self.train_mode = True
        self.hint_bad = self.step_zero[10:11]              # a caller's token-count hint contradicted the mask (step.py)
        self.pack_text = self.opt.pack_text                 # drop the rows of padding tokens from the passes that only read position 0 (step.py)
        self.layer_done_cb = None
        # the unimodal text and PV chains (and their backward) are independent: run them on two HIP streams so the small-M
        # kernels of one fill the CUs the other leaves idle (S1: 13.8 k rows = 162 of 256 CUs per 256x256-tile GEMM wave)
        self.multi_stream = self.opt.multi_stream
        self.wgrad_async = self.opt.wgrad_stream and self.multi_stream
        # Batches whose every chain fills the chip by itself (B x Lt above STREAM_TOKENS_MAX) run on ONE stream: side streams gain
        # nothing there (412 vs 408 ms per step at B = 512, Lt = 256) and every stream keeps its own allocator pool -- 228 GB peak /
        # 286 GB reserved of 288 on three streams (one allocator retry = a multi-second step) against 160 / 207 GB on one.
        self._one_stream = False
        # A stream takes its hardware queue at its FIRST USE and there are only a handful of queues: a foreign stream first used between
        # side0 and side1 ran the plain step at 71.6 ms instead of 59.4 (tools/first_steps.py, EXPERIMENTS.md 2.7b).  So the step's
        # streams take their queues here, in one go.  (Data-parallel processes do it in parallel.grad_sync_fn, RCCL's stream first.)
        # (A process that merely HOLDS a one-rank group -- torchrun --nproc 1, user code -- gets no exchange from grad_sync_fn and so no
        # binding there: what decides is whether a data-parallel exchange will run, not whether torch.distributed is initialised.)
        dist_ = torch.distributed
        will_exchange = dist_.is_available() and dist_.is_initialized() and (dist_.get_world_size() > 1 or self.opt.force_dist)
        # data-parallel runs with EngineOptions.dp_four_streams: the momentum chains share side stream 0 with the text student chain
        self._one_side = bool(will_exchange and self.opt.dp_four_streams)
        if self.multi_stream and torch.device(device).type == "cuda" and not ops._DRY_RUN and not will_exchange:
            streams.bind_in_order(device, ("side0", "side1", "wgrad"))
        self.force_one_stream = False     # set by the data-parallel schedule check (model.py::_schedule_check)
        self._wg_stream, self._wg_pending, self._wg_keep = None, False, []
        self._salt = 0
        self._off_path_ok, self._pre_bwd = False, None     # (set per step by SPMM.fused_step: single-rank runs, data-parallel ones with dp_four_streams)
        self._xattn_checked = self._xattn_off = False       # fused cross-attention: one-time self-check done / failed (_attn_block_fwd)
        self.tape = None
        E, Q = cfg.embed_dim, cfg.queue_size
        self._bank = None          # queue GEMM shadows, sized on first use (depend on the local batch)

    # ------------------------------------------------------------------------------------------------ helpers
    def _fork(self, which: int = 0):
        """-> side stream `which` that waits for everything enqueued so far on the current stream (None: single-stream mode)."""
        if not self.multi_stream or self._one_stream or self.dev.type != "cuda" or ops._DRY_RUN:
            return None
        side = streams.get(self.dev, "side0" if self._one_side else f"side{which}")        # process-wide: every model of a process shares the same streams
        streams.after(side, torch.cuda.current_stream())
        return side

    def _join(self, side):
        if side is not None:
            streams.after(torch.cuda.current_stream(), side)

    @staticmethod
    def _on(side):
        return torch.cuda.stream(side) if side is not None else contextlib.nullcontext()

    def _new(self, *shape, dtype=BF):
        return torch.empty(*shape, dtype=dtype, device=self.dev)

    def _stats(self, M, save):
        """-> (mean, rstd) fp32 [M] of a LayerNorm whose backward will run, (None, None) otherwise."""
        return (self._new(M, dtype=torch.float32), self._new(M, dtype=torch.float32)) if save else (None, None)

    def _zeros(self, *shape, dtype=BF):
        return ops.zero_(torch.empty(*shape, dtype=dtype, device=self.dev))

    def _next_salt(self):
        self._salt += 1
        return self._salt * 0x9E3779B97F4A7C15 % (1 << 63)

    def _p_hidden(self, c: BertConfig):
        return c.hidden_dropout_prob if self.train_mode else 0.0

    def _p_attn(self, c: BertConfig):
        return c.attention_probs_dropout_prob if self.train_mode else 0.0

    def _wT(self, key, src_fp32):
        return self.P.wT(key, src_fp32)

    def _wgrad(self, dY, X, gW, gb=None, inline=False, md=None):
        """gW[N,K] += dY[M,N]^T X[M,K] ; gb[N] += column sums of dY (TN GEMM: no transposed copies).  md: device-side row count of dY / X.
        Nothing on the backward's critical path reads a weight gradient, so (unless `inline`) the two launches go to a side stream
        behind an event on the current one: they fill the CUs the data-gradient chain leaves idle (attention / LayerNorm backward,
        tails of small-M GEMMs).  All weight gradients share ONE such stream (accumulations into the same tensor stay ordered);
        `wgrad_join()` makes the current stream wait for it (before a layer's gradient exchange, before the optimiser)."""
        ws = None if inline else self._wgrad_side()
        C = gW.view(dY.shape[1], X.shape[1])
        if ws is None:
            if gb is not None:
                ops.colsum_bf16(dY, gb, R_dev=md)
            ops.gemm_tn(dY, X, C, M_dev=md)
            return
        streams.after(ws, torch.cuda.current_stream())
        with torch.cuda.stream(ws):
            if gb is not None:
                ops.colsum_bf16(dY, gb, R_dev=md)
            ops.gemm_tn(dY, X, C, M_dev=md)
        # The operands must outlive the side stream's use of them.  They are simply kept referenced until the next join
        # (`record_stream` on ~100 tensors per step makes the caching allocator poll events on every allocation).
        self._wg_keep.append((dY, X))
        self._wg_pending = True

    def _wgrad_side(self):
        if not self.wgrad_async or self._one_stream or self.dev.type != "cuda" or ops._DRY_RUN:
            return None
        self._wg_stream = streams.get(self.dev, "wgrad")
        return self._wg_stream

    def off_path(self, fn):
        """Maintenance that nothing needs before the next BACKWARD -- zeroing the gradient arena, rebuilding the transposed weight shadows
        of the data-gradient GEMMs after the optimiser -- runs on the weight-gradient stream (idle during the forward) behind everything
        enqueued so far; `backward()` waits for it.  Inline when that stream is not in use (one-stream schedule, data-parallel runs: their
        stream order is part of the schedule) or while a graph is being captured."""
        ws = self._wgrad_side() if self._off_path_ok else None
        if ws is None or torch.cuda.is_current_stream_capturing():
            fn()
            return
        streams.after(ws, torch.cuda.current_stream())
        with torch.cuda.stream(ws):
            fn()
            self._pre_bwd = streams.mark(ws)

    def pre_backward_wait(self):
        ev, self._pre_bwd = self._pre_bwd, None
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def wgrad_join(self, release: bool = False):
        """The current stream waits for every weight-gradient launch issued so far."""
        if self._wg_stream is not None and self._wg_pending:
            streams.after(torch.cuda.current_stream(), self._wg_stream)
            if release:                               # the current stream is now ordered behind every use: the blocks may go back to it
                self._wg_keep.clear()
                self._wg_pending = False

    def end_backward(self):
        """The weight gradients of the side stream are complete from here on; their operands and the tape are released."""
        self.wgrad_join(release=True)
        self.tape = None

    def _pack_plan(self, mask32: torch.Tensor, B: int, Lt: int, n_tokens: Optional[int] = None):
        """Row bookkeeping for the packed text passes: valid rows of the dense [B*Lt] layout in order, per-sequence start
        and length.  The packed row count sizes the GEMMs, so the host must know it: either the data pipeline says so
        (`n_tokens`: the tokenizer's attention mask is a host tensor, its sum costs nothing there -- and the caller then vouches
        that every mask row is a non-empty prefix, which is what padding='longest' produces) or it is read back from the device,
        one blocking read per step.  Returns None -- dense fallback -- when a sequence does not start with a valid token
        (position 0 is what the losses read) or nothing would be saved."""
        if n_tokens is not None:
            M = int(n_tokens)
            if M >= B * Lt:
                return None
            # The caller vouches for the hint (SPMM.training_step derives it from the tokenizer's host mask itself).  Best effort
            # against a wrong one, without a read-back: the mismatch is detected on the device (spmm_pack_plan raises `hint_bad`) and
            # raises the NaN flag (AdamW, EMA and enqueue become no-ops, as for a non-finite loss, SPMM_models.py:132-134), and the
            # per-sequence bookkeeping is clamped to the rows the hint sized; launches sized from other derived quantities may still misbehave.
        else:
            lens = mask32.sum(1)
            prefix = (torch.arange(Lt, device=mask32.device)[None, :] < lens[:, None]) == (mask32 != 0)
            stats = torch.stack([lens.sum(), (lens > 0).sum(), prefix.all().to(lens.dtype)]).cpu()
            M, nonempty, is_prefix = int(stats[0]), int(stats[1]), int(stats[2])
            if nonempty != B or not is_prefix or M >= B * Lt:   # holes in the mask: the packed index would not be the position
                return None
        if M < 1:
            return None
        # valid rows first, original order kept; whatever the hint was, no index leaves the M rows it sized (csrc/plan.hip)
        return ops.pack_plan(mask32, M, self.hint_bad)

    def text_rows(self, x: torch.Tensor, mask32: torch.Tensor, pk: Optional[dict]):
        """The embedded text x (dense [B*L, H]) as ONE group of B sequences for the text layers -> (rows, Batch, int64 [B]: the row of
        position 0 of every sequence): the valid rows of the pack plan `pk` (padding rows dropped), or -- pk None -- the dense rows
        under their key mask."""
        B, L = mask32.shape
        if not pk:
            return x, Batch([Group(0, B, L, mask32, B)]), torch.arange(B, dtype=torch.int64, device=self.dev) * L
        x = ops.gather_rows2(self._new(pk["M"], x.shape[1]), x, pk["rows"])
        return x, Batch([Group(0, B, L, None, B, q_row0=pk["row0"], q_len=pk["len"], nrows=pk["M"])]), pk["row0_64"]

    def text_rows_of(self, pfx, c, ids32, mask32, *, n_tokens: Optional[int] = None, save=False, causal=False, what: str = "") -> TextRows:
        """The text pass of every path that encodes SMILES rows, up to the layers: embeddings of the token ids (int32 [B, L] on the
        device), the pack plan wherever the packed attention layouts hold the length (`n_tokens`: the host's count of valid tokens, which
        spares the plan its device read), the rows as ONE group -- causal from sequence 0 with `causal`.  `what` prefixes the error."""
        B, L = ids32.shape
        if L > c.max_position_embeddings:
            raise ValueError(f"{what}sequence length {L} exceeds the {c.max_position_embeddings} position embeddings")
        x, esv = self.embed_text(pfx, c, ids32, B, L, save)
        pk = self._pack_plan(mask32, B, L, n_tokens) if (self.pack_text and L <= ops.ATTN_MAXL) else None
        x, groups, cls_rows = self.text_rows(x, mask32, pk)
        if causal:
            groups.groups[0].causal_from = 0
        return TextRows(x, groups, pk, cls_rows, ids32, mask32, B, L, esv)

    def encode_text(self, pfx, c, ids32, mask32, *, n_tokens: Optional[int] = None, save=False, causal=False, what: str = "") -> TextRows:
        """`text_rows_of`, then the unimodal layers 0 .. fusion_layer - 1 over the rows: fills `y` and `tape`."""
        t = self.text_rows_of(pfx, c, ids32, mask32, n_tokens=n_tokens, save=save, causal=causal, what=what)
        t.y, t.tape, _ = self.stack_fwd(pfx, c, range(0, c.fusion_layer), False, t.x, t.groups, save)
        return t

    # ---------------------------------------------------------------------------------------- attention block
    def _ln_res(self, x, X, X32, gamma, beta, y, md, **kw):
        """y = LN(dropout(x) + residual): the residual is X (bf16) or, with the fp32 residual stream (EngineOptions.resid_fp32), X32;
        returns the fp32 twin of y in that mode (None otherwise)."""
        if X32 is None:
            ops.ln_fwd(x, X, gamma, beta, y, rows_dev=md, **kw)
            return None
        assert md is None                                        # (spmm_ln_fwd_r32 takes no device-side row count)
        y32 = self._new(*y.shape, dtype=torch.float32)
        ops.ln_fwd_r32(x, X32, gamma, beta, y, y32=y32, **kw)
        return y32

    def _proj_ln(self, op, A, resid, X32, *, save, eps, ph, salt, md=None):
        """y = LayerNorm(dropout(A W^T + b) + resid): BertSelfOutput / BertOutput (xbert.py:369-373, 447-451) with the parameters
        `op`dense.* / `op`LayerNorm.*: the projection GEMM, then dropout + residual + LayerNorm in one row kernel (the pre-norm sum z is
        formed in fp32 registers; its bf16 copy is kept for the backward, which regenerates the dropout mask from (seed, salt)).
        md: device-side row count of A.  -> (y, LnTape, fp32 twin of y or None); `_proj_ln_bwd` is the backward."""
        P = self.P
        Wb = P.wb(op + "dense.weight")
        M, H = A.shape[0], Wb.shape[0]
        x, y = self._new(M, H), self._new(M, H)
        mean, rstd = self._stats(M, save)
        ops.gemm_nt(A, Wb, x, bias=P.w(op + "dense.bias"), M_dev=md)
        # The backward recovers the normalised values from the OUTPUT y (spmm_ln_bwd, beta_from_y): the pre-norm sum is not stored -- one
        # write pass per residual LayerNorm less, and the projection's output buffer is free again at once (EngineOptions.ln_from_y;
        # the fp32 residual stream keeps the stored sum)
        from_y = self.opt.ln_from_y and X32 is None
        y32 = self._ln_res(x, resid, X32, P.w(op + "LayerNorm.weight"), P.w(op + "LayerNorm.bias"), y, md,
                           zout=x if (save and not from_y) else None, mean=mean, rstd=rstd, eps=eps, dropout_p=ph, seed=self.seed, salt=salt)
        return y, LnTape(None if from_y else x, y, mean, rstd, salt), y32

    def _proj_ln_bwd(self, op, tape, dY, A, ph, md=None):
        """Backward of `_proj_ln` (or of the fused cross-attention launch, which fills the same record) up to the projection's output:
        -> (dz, dx) = gradient of the residual branch, gradient of the projection's output (one tensor when hidden dropout is off).  The
        LayerNorm, projection-bias and projection-weight gradients are accumulated; the data-gradient GEMM on dx stays with the caller."""
        P, (M, H) = self.P, dY.shape
        dz = self._new(M, H)
        dx = self._new(M, H) if ph > 0 else dz
        from_y = tape.z is None                           # (the forward kept no pre-norm sum: normalised values from the output, _proj_ln)
        ops.ln_bwd(dY, tape.y if from_y else tape.z, tape.mean, tape.rstd, P.w(op + "LayerNorm.weight"), dz, dx=dx if ph > 0 else None,
                   dgamma=P.g(op + "LayerNorm.weight"), dbeta=P.g(op + "LayerNorm.bias"), dropout_p=ph, seed=self.seed, salt=tape.salt,
                   dxsum=P.g(op + "dense.bias"), rows_dev=md, beta_from_y=P.w(op + "LayerNorm.bias") if from_y else None)
        self._wgrad(dx, A, P.g(op + "dense.weight"), md=md)
        return dz, dx

    def _attn_block_fwd(self, pfx, c, X, groups, save, cross, X32=None, kv_tap=None, xattn_tap=None):
        """BertAttention.forward xbert.py:401-422 on a token batch.  cross=True uses the groups' key/value sources.
        kv_tap (self-attention only): called with the fused Q|K|V projection [M, 3H] right after it is formed (`stack_fwd`).
        xattn_tap (cross-attention only): called per group with its projected query rows and its source's keys (`stack_fwd`).
        -> (y, tape entry, fp32 twin of y or None)."""
        P, H, nH = self.P, c.hidden_size, c.num_attention_heads
        # Every form of the block draws its salts here, in one order (every group's attention salt, then the hidden one): the composite of
        # launches, the fused one-launch form and the composite that replaces a fused form that failed its self-check draw the same masks
        salts_a = [self._next_salt() for _ in groups]
        salt_h = self._next_salt()
        sv = {"X": X, "salt_a": salts_a, "cross": cross}
        if not cross:
            ctx, core = self._self_attn_fwd(pfx, c, X, groups, save, salts_a, kv_tap)
        else:
            sv["Qc"] = Qc = ops.gemm_nt(X, P.wb(pfx + ".self.query.weight"), self._new(X.shape[0], H), bias=P.w(pfx + ".self.query.bias"),
                                        M_dev=groups.rows_dev)
            done = {id(g.src): g.src.proj[pfx] for g in groups if g.src is not None and g.src.proj and pfx in g.src.proj}
            kv_of = functools.partial(self._xattn_kv, P.fused(pfx + ".self.", ("key", "value"), "weight"),
                                      P.fused(pfx + ".self.", ("key", "value"), "bias", what="w"), done)
            if xattn_tap is not None:
                # views of what both forms of the block read below: no copy, no salt, no launch.  (kv_of caches per source, so the
                # block's own kv_of(g) returns the very tensor the tap saw.)
                for gi, g in enumerate(groups):
                    xattn_tap(gi, g, Qc[g.rows], kv_of(g)[:, :H])
            fx = self.opt.fused_xattn
            fused = ((fx is True or fx == "all" or (fx == "nograd" and not save)) and not self._xattn_off and X32 is None
                     and groups.rows_dev is None and all(ops.xattn_supported(H, nH, g.L, g.Lkv) for g in groups))
            if fused:
                y, out = self._xattn_fused_fwd(pfx, c, X, Qc, kv_of, groups, save, salts_a, salt_h)
                g0 = groups.groups[0]
                if not self._xattn_checked and not ops._DRY_RUN and g0.row0 == 0:
                    self._xattn_checked = True
                    agrees, dmax, dmean = self._xattn_agrees(pfx, c, X, Qc, out["KV"][0], g0, y, salts_a[0], salt_h)
                    if not agrees:
                        # Not fatal: the composite of launches is always available.  This process stops using the one-launch form and says
                        # so (a default path must not be able to end a run; the kernel's own parity tests compare it directly).  The
                        # composite below runs with the salts drawn above: from here on the masks are those of fused_xattn="off".
                        import warnings
                        warnings.warn(f"spmm_amd: the fused cross-attention kernel disagrees with the composite launches (max |dy| {dmax:.3g}, "
                                      f"mean {dmean:.3g}); falling back to the composite for this process (SPMM_FUSED_XATTN=off)")
                        streams.note("fused cross-attention kernel failed its one-time self-check: composite launches used instead")
                        self._xattn_off = True
                        fused = False
                if fused:
                    sv.update(out)
                    return y, (sv if save else None), None
            ctx, core = self._xattn_core_fwd(c, Qc, kv_of, groups, save, salts_a)
        y, ln, y32 = self._proj_ln(pfx + ".output.", ctx, X, X32, save=save, eps=c.layer_norm_eps, ph=self._p_hidden(c), salt=salt_h,
                                   md=groups.rows_dev)
        sv.update(core, ctx=ctx, ln=ln)
        return y, (sv if save else None), y32

    def _self_attn_fwd(self, pfx, c, X, groups, save, salts, kv_tap=None):
        """Self-attention core: the fused Q/K/V projection of the batch, then one attention launch per group.  -> (ctx, tape fields)"""
        P, H, nH, M = self.P, c.hidden_size, c.num_attention_heads, X.shape[0]
        Wqkv = P.fused(pfx + ".self.", ("query", "key", "value"), "weight")
        bqkv = P.fused(pfx + ".self.", ("query", "key", "value"), "bias", what="w")
        QKV = ops.gemm_nt(X, Wqkv, self._new(M, 3 * H), bias=bqkv, M_dev=groups.rows_dev)
        if kv_tap is not None:
            kv_tap(QKV)
        ctx, lses = self._new(M, H), []
        skv = {}                                                 # K/V of the groups' private self-attention sources (SelfKV), one GEMM each
        for g, salt in zip(groups, salts):
            lse = self._new(g.nseq, nH, g.L, dtype=torch.float32) if save else None
            r = g.rows
            kw = dict(nseq=g.nseq, nH=nH, Lq=g.L, dropout_p=self._p_attn(c), seed=self.seed, salt=salt, q_row0=g.q_row0, q_len=g.q_len)
            if g.self_src is not None:
                # query rows = a subset of their sequences' rows (here: position 0 only); keys / values = every token of the
                # sequence, projected from the layer input with the key / value rows of the fused weight
                if id(g.self_src) not in skv:
                    skv[id(g.self_src)] = ops.gemm_nt(g.self_src.x, Wqkv[H:], self._new(g.self_src.x.shape[0], 2 * H), bias=bqkv[H:],
                                                      M_dev=g.self_src.rows_dev)
                KVs = skv[id(g.self_src)]
                ops.attn_fwd_long(QKV[r, :H], KVs[:, :H], KVs[:, H:], ctx[r], lse, Lkv=g.skv_L, kmask=None, causal_from=g.nseq,
                                  kv_row0=g.skv_row0, kv_len=g.skv_len, **kw)
            else:
                ops.attn_fwd_long(QKV[r, :H], QKV[r, H:2 * H], QKV[r, 2 * H:], ctx[r], lse, Lkv=g.L, kmask=g.kmask, causal_from=g.causal_from,
                                  kv_row0=g.q_row0, kv_len=g.q_len, **kw)
            lses.append(lse)
        return ctx, dict(QKV=QKV, SKV=skv, lse=lses)

    def _xattn_kv(self, Wkv, bkv, done, g):
        """Projected keys | values [source rows, 2H] of group g's cross-attention source; a shared source (KVSource) is projected once per
        layer (`done`: what this block has projected so far)."""
        key, kv = (id(g), g.kv) if g.src is None else (id(g.src), g.src.kv)
        if key not in done:
            done[key] = ops.gemm_nt(kv, Wkv, self._new(kv.shape[0], Wkv.shape[0]), bias=bkv)
        return done[key]

    def _xattn_core_fwd(self, c, Qc, kv_of, groups, save, salts):
        """Composite cross-attention core: per group the key/value projection of its source (if new), then the attention launch.
        -> (ctx, tape fields)"""
        H, nH = c.hidden_size, c.num_attention_heads
        ctx, KVs, lses = self._new(Qc.shape[0], H), [], []
        for g, salt in zip(groups, salts):
            KV = kv_of(g)
            lse = self._new(g.nseq, nH, g.L, dtype=torch.float32) if save else None
            ops.attn_fwd_long(Qc[g.rows], KV[:, :H], KV[:, H:], ctx[g.rows], lse, nseq=g.nseq, nH=nH, Lq=g.L, Lkv=g.Lkv, is_cross=True,
                              dropout_p=self._p_attn(c), seed=self.seed, salt=salt, **g.cross_layout())
            KVs.append(KV)
            lses.append(lse)
        return ctx, dict(KV=KVs, lse=lses)

    def _xattn_fused_fwd(self, pfx, c, X, Qc, kv_of, groups, save, salts, salt_h):
        """The cross-attention block as ONE launch per group for core + output projection + dropout + residual + LayerNorm
        (csrc/xattn.hip), behind the same projections as the composite.  -> (y, tape fields)"""
        P, H, nH, M = self.P, c.hidden_size, c.num_attention_heads, X.shape[0]
        y = self._new(M, H)
        z, ctx = (self._new(M, H), self._new(M, H)) if save else (None, None)
        mean, rstd = self._stats(M, save)
        WoF = P.wF(pfx + ".output.dense.weight")
        KVs, lses = [], []
        for g, salt in zip(groups, salts):
            KV = kv_of(g)
            lse = self._new(g.nseq, nH, g.L, dtype=torch.float32) if save else None
            r = g.rows
            ops.xattn_fwd(Qc[r], KV[:, :H], KV[:, H:], WoF, P.w(pfx + ".output.dense.bias"), X[r], P.w(pfx + ".output.LayerNorm.weight"),
                          P.w(pfx + ".output.LayerNorm.bias"), y[r], nseq=g.nseq, nH=nH, Lq=g.L, Lkv=g.Lkv, eps=c.layer_norm_eps,
                          Z=None if z is None else z[r], mean=None if mean is None else mean[r.start:r.stop],
                          rstd=None if rstd is None else rstd[r.start:r.stop], CTX=None if ctx is None else ctx[r], lse=lse,
                          attn_dropout_p=self._p_attn(c), salt_a=salt, hidden_dropout_p=self._p_hidden(c), salt_h=salt_h, seed=self.seed,
                          row_base=r.start, **g.cross_layout())
            KVs.append(KV)
            lses.append(lse)
        return y, dict(KV=KVs, lse=lses, ctx=ctx, ln=LnTape(z, y, mean, rstd, salt_h))

    def _xattn_agrees(self, pfx, c, X, Qc, KV, g, y, salt_a, salt_h):
        """One-time self-check of the fused kernel: its output `y` on the rows of group g (the batch's first rows) against the composite
        launches with the same dropout masks (same seed, salts and row counter).  The kernel keeps asynchronously loaded registers in
        flight behind hand-counted waits: a compiler change that broke that would corrupt y silently.  A host read.
        -> (agrees, max |dy|, mean |dy|)"""
        H, r = c.hidden_size, g.rows
        c2 = self._new(r.stop, H)
        ops.attn_fwd_long(Qc[r], KV[:, :H], KV[:, H:], c2, None, nseq=g.nseq, nH=c.num_attention_heads, Lq=g.L, Lkv=g.Lkv, is_cross=True,
                          dropout_p=self._p_attn(c), seed=self.seed, salt=salt_a, **g.cross_layout())
        y2, _, _ = self._proj_ln(pfx + ".output.", c2, X[r], None, save=False, eps=c.layer_norm_eps, ph=self._p_hidden(c), salt=salt_h)
        d = (y[r].float() - y2.float()).abs()
        dmax, dmean = float(d.max()), float(d.mean())
        scale = max(1.0, float(y2.float().abs().max()) / 8.0)              # (outlier channels of a trained model scale the roundings)
        return dmax < 0.25 * scale and dmean < 5e-3 * scale, dmax, dmean    # (bf16 roundings of x differ: ~1e-3 on average)

    def _attn_block_bwd(self, pfx, c, sv, dY, groups, dkv_acc):
        """-> dX (bf16).  Parameter gradients accumulate into the flat grad arena; cross-attention key/value source
        gradients accumulate (fp32) into dkv_acc[i] for group i."""
        P, H, nH = self.P, c.hidden_size, c.num_attention_heads
        X, M, md = sv["X"], sv["X"].shape[0], groups.rows_dev
        pa, ph = self._p_attn(c), self._p_hidden(c)
        dz, dx = self._proj_ln_bwd(pfx + ".output.", sv["ln"], dY, sv["ctx"], ph, md)
        dctx = self._new(M, H)
        ops.gemm_nt(dx, self._wT(pfx + ".output.dense", P.w(pfx + ".output.dense.weight")), dctx, M_dev=md)
        dX = self._new(M, H)
        if not sv["cross"]:
            QKV = sv["QKV"]
            dQKV = self._new(M, 3 * H)
            gWqkv = P.fused(pfx + ".self.", ("query", "key", "value"), "weight", what="g")
            gbqkv = P.fused(pfx + ".self.", ("query", "key", "value"), "bias", what="g")
            dskv = {}
            for i, g in enumerate(groups):
                r = g.rows
                kw = dict(nseq=g.nseq, nH=nH, Lq=g.L, dropout_p=pa, seed=self.seed, salt=sv["salt_a"][i], q_row0=g.q_row0, q_len=g.q_len)
                if g.self_src is not None:
                    if id(g.self_src) not in dskv:               # rows no sequence owns (zero rows past a negative's length) stay zero
                        dskv[id(g.self_src)] = (g.self_src, self._zeros(g.self_src.x.shape[0], 2 * H))
                    KVs, dKVs = sv["SKV"][id(g.self_src)], dskv[id(g.self_src)][1]
                    ops.attn_bwd_long(QKV[r, :H], KVs[:, :H], KVs[:, H:], sv["ctx"][r], sv["lse"][i], dctx[r], dQKV[r, :H], dKVs[:, :H], dKVs[:, H:],
                                      Lkv=g.skv_L, kmask=None, causal_from=g.nseq, kv_row0=g.skv_row0, kv_len=g.skv_len, **kw)
                    ops.zero_(dQKV[r, H:])                       # the batch rows' own keys / values were never attended
                    continue
                ops.attn_bwd_long(QKV[r, :H], QKV[r, H:2 * H], QKV[r, 2 * H:], sv["ctx"][r], sv["lse"][i], dctx[r], dQKV[r, :H],
                                  dQKV[r, H:2 * H], dQKV[r, 2 * H:], Lkv=g.L, kmask=g.kmask, causal_from=g.causal_from,
                                  kv_row0=g.q_row0, kv_len=g.q_len, **kw)
            self._wgrad(dQKV, X, gWqkv, gbqkv, md=md)
            WT = self._wT(pfx + ".self.qkv", P.fused(pfx + ".self.", ("query", "key", "value"), "weight", what="w"))
            for src, dKVs in dskv.values():                      # key / value projections of the private sources: weight and data gradient
                self._wgrad(dKVs, src.x, gWqkv[H:], gbqkv[H:], md=src.rows_dev)
                ops.gemm_nt(dKVs, WT[:, H:], src.dx, M_dev=src.rows_dev)
            ops.gemm_nt(dQKV, WT, dX, R=dz, M_dev=md)
        else:
            Qc = sv["Qc"]
            dQc = self._new(M, H)
            gWkv = P.fused(pfx + ".self.", ("key", "value"), "weight", what="g")
            gbkv = P.fused(pfx + ".self.", ("key", "value"), "bias", what="g")
            WkvT = self._wT(pfx + ".self.kv", P.fused(pfx + ".self.", ("key", "value"), "weight", what="w"))
            pool = {}                                            # per shared source: the consumers' dK/dV, dense per query sequence
            for i, g in enumerate(groups):
                r = g.rows
                KV = sv["KV"][i]
                src = g.src
                if src is not None:
                    if id(src) not in pool:
                        pool[id(src)] = (src, self._new(src.nseq * src.Lkv, 2 * H))
                    dKV = pool[id(src)][1][g.kv_off * g.Lkv:(g.kv_off + g.nseq) * g.Lkv]
                else:
                    dKV = self._new(g.nseq * g.Lkv, 2 * H)
                ops.attn_bwd_long(Qc[r], KV[:, :H], KV[:, H:], sv["ctx"][r], sv["lse"][i], dctx[r], dQc[r], dKV[:, :H], dKV[:, H:],
                                  nseq=g.nseq, nH=nH, Lq=g.L, Lkv=g.Lkv, is_cross=True, dropout_p=pa, seed=self.seed, salt=sv["salt_a"][i],
                                  **g.cross_layout())
                if src is None:
                    self._wgrad(dKV, g.kv, gWkv, gbkv)
                    ops.gemm_nt(dKV, WkvT, dkv_acc[i], epi=ops.EPI_F32_ACC)
            for src, dKV in pool.values():                       # fold onto the unique source rows, then one wgrad + dgrad
                W = src.Lkv * 2 * H
                dKVu = ops.segment_sum_bf16(dKV.view(src.nseq, W), src.start, src.list, self._new(src.U, W)).view(-1, 2 * H)
                if src.pack_idx is not None:
                    dKVu = ops.gather_rows(self._new(src.pack_idx.numel(), 2 * H), dKVu, src.pack_idx)
                self._wgrad(dKVu, src.kv, gWkv, gbkv)
                ops.gemm_nt(dKVu, WkvT, dkv_acc[id(src)], epi=ops.EPI_F32_ACC)
            self._wgrad(dQc, X, P.g(pfx + ".self.query.weight"), P.g(pfx + ".self.query.bias"), md=md)
            ops.gemm_nt(dQc, self._wT(pfx + ".self.query", P.w(pfx + ".self.query.weight")), dX, R=dz, M_dev=md)
        return dX

    # ------------------------------------------------------------------------------------------------- layers
    def _layer_fwd(self, lp, c, has_cross, X, groups, save, X32=None, kv_tap=None, xattn_tap=None):
        """BertLayer.forward xbert.py:469-534.  -> (y, tape entry, fp32 twin of y or None)."""
        P, H, I, M = self.P, c.hidden_size, c.intermediate_size, X.shape[0]
        tap = {} if kv_tap is None else {"kv_tap": kv_tap}       # (without a tap the call is the one it always was: bench.py wraps this method)
        a, sv1, a32 = self._attn_block_fwd(lp + "attention", c, X, groups, save, cross=False, X32=X32, **tap)
        sv2 = None
        if has_cross:
            xtap = {} if xattn_tap is None else {"xattn_tap": xattn_tap}
            a, sv2, a32 = self._attn_block_fwd(lp + "crossattention", c, a, groups, save, cross=True, X32=a32, **xtap)
        h = self._new(M, I)
        # backward needs only gelu'(pre-activation): the forward epilogue stores it (it shares the exponential with the erf) and the
        # backward epilogue is a plain multiply -- the erf / exp work of xbert.py:436's backward leaves the dgrad GEMM
        dact = self._new(M, I) if save else None
        ops.gemm_nt(a, P.wb(lp + "intermediate.dense.weight"), h, bias=P.w(lp + "intermediate.dense.bias"),
                    epi=ops.EPI_GELU_DERIV if save else ops.EPI_GELU, C2=dact, M_dev=groups.rows_dev)
        salt = self._next_salt()
        y, ln, y32 = self._proj_ln(lp + "output.", h, a, a32, save=save, eps=c.layer_norm_eps, ph=self._p_hidden(c), salt=salt, md=groups.rows_dev)
        sv = dict(att=sv1, cross=sv2, a=a, h=h, dact=dact, ln=ln) if save else None
        return y, sv, y32

    def _layer_bwd(self, lp, c, sv, dY, groups, dkv_acc):
        P, H, I, M, md = self.P, c.hidden_size, c.intermediate_size, dY.shape[0], groups.rows_dev
        dz, dx = self._proj_ln_bwd(lp + "output.", sv["ln"], dY, sv["h"], self._p_hidden(c), md)
        dpre = self._new(M, I)
        ops.gemm_nt(dx, self._wT(lp + "output.dense", P.w(lp + "output.dense.weight")), dpre,
                    epi=ops.EPI_MUL, G=sv["dact"], colsum=P.g(lp + "intermediate.dense.bias"), M_dev=md)
        self._wgrad(dpre, sv["a"], P.g(lp + "intermediate.dense.weight"), md=md)
        da = self._new(M, H)
        ops.gemm_nt(dpre, self._wT(lp + "intermediate.dense", P.w(lp + "intermediate.dense.weight")), da, R=dz, M_dev=md)
        if sv["cross"] is not None:
            da = self._attn_block_bwd(lp + "crossattention", c, sv["cross"], da, groups, dkv_acc)
        return self._attn_block_bwd(lp + "attention", c, sv["att"], da, groups, None)

    def stack_fwd(self, pfx, c, layers, has_cross, X, groups, save, X32=None, kv_tap=None, xattn_tap=None):
        """groups: the Batch X holds.  -> (y, tape, y32).  With X32 (the fp32 twin of X: EngineOptions.resid_fp32) the residual stream runs
        in fp32 and y32 is the fp32 twin of y (None otherwise).  kv_tap(layer index, QKV [M, 3H]) is called with every layer's
        self-attention Q|K|V projection right after it is formed (decode.CachedDecoder.prefill fills its K/V cache from it); None, the
        default, changes nothing -- no launch, no salt.  xattn_tap(layer index, group index, group, Q rows of the group [rows, H],
        K of its source [source rows, H]) is called once per cross-attention group of every layer that has a cross-attention block, right
        after the group's K/V projection is available, on the composite and on the one-launch form alike (attribution.py reads the
        attention probabilities from these views); None, the default: the calls below are the ones they always were."""
        tape = []
        for i in layers:
            tap = None if kv_tap is None else functools.partial(kv_tap, i)
            xtap = {} if xattn_tap is None else {"xattn_tap": functools.partial(xattn_tap, i)}
            X, sv, X32 = self._layer_fwd(f"{pfx}encoder.layer.{i}.", c, has_cross and i >= c.fusion_layer, X, groups, save, X32=X32, kv_tap=tap,
                                         **xtap)
            tape.append(sv)
        return X, tape, X32

    def stack_bwd(self, pfx, c, layers, tape, dY, groups, dkv_acc=None):
        for i, sv in zip(reversed(list(layers)), reversed(tape)):
            dY = self._layer_bwd(f"{pfx}encoder.layer.{i}.", c, sv, dY, groups, dkv_acc)
            if self.layer_done_cb is not None:           # this layer's gradients are final: data-parallel reduce may start
                self._layer_done(f"{pfx}encoder.layer.{i}.")
        return dY

    def _layer_done(self, prefix):
        """Hand a finished layer's slice to the gradient exchange.  While slices are exchanged the weight gradients run on the
        backward's own stream (SPMM.fused_step), so the stream calling this is ordered behind every writer of the slice."""
        ws = self._wg_stream if (self._wg_pending and self.wgrad_async) else None
        if ws is None:
            self.wgrad_join()
            return self.layer_done_cb(prefix)
        # asynchronous weight gradients beside the exchange (EngineOptions.dp_four_streams): the slice is final once the weight-gradient stream
        # AND the stream this layer's backward ran on are done with it -- the collective is issued from the weight-gradient stream behind an
        # event on the current one (ProcessGroupNCCL orders RCCL's stream behind the issuing stream); the backward itself does not wait
        streams.after(ws, torch.cuda.current_stream())
        with torch.cuda.stream(ws):
            return self.layer_done_cb(prefix)

    # --------------------------------------------------------------------------------------------- embeddings
    def _embed(self, mode, pfx, c, nseq, L, save, salt, **src):
        """One spmm_embed_ln_fwd launch: BertEmbeddings' position / type / LayerNorm parameters of `pfx` around the mode's sources (`src`).
        -> (y, LnTape)"""
        P, H = self.P, c.hidden_size
        y = self._new(nseq * L, H)
        z = self._new(nseq * L, H) if save else None
        mean, rstd = self._stats(nseq * L, save)
        ops.embed_ln_fwd(mode, y, nseq=nseq, L=L, H=H, pos=P.w(pfx + "embeddings.position_embeddings.weight"),
                         type0=P.w(pfx + "embeddings.token_type_embeddings.weight"), gamma=P.w(pfx + "embeddings.LayerNorm.weight"),
                         beta=P.w(pfx + "embeddings.LayerNorm.bias"), zout=z, mean=mean, rstd=rstd, eps=c.layer_norm_eps,
                         dropout_p=self._p_hidden(c), seed=self.seed, salt=salt, **src)
        return y, LnTape(z, None, mean, rstd, salt)

    def embed_text(self, pfx, c, ids32, nseq, L, save):
        return self._embed(0, pfx, c, nseq, L, save, self._next_salt(), ids=ids32, word=self.P.w(pfx + "embeddings.word_embeddings.weight"))

    def embed_pv(self, pfx, c, prop, mpm_mask, nseq, src_mod, save):
        P = self.P
        return self._embed(1, pfx, c, nseq, self.cfg.n_props + 1, save, self._next_salt(), pv_x=prop, pv_mask=mpm_mask,
                           pv_w=P.w("property_embed.weight"), pv_b=P.w("property_embed.bias"), pv_cls=P.w("property_cls"),
                           pv_masktok=P.w("property_mask"), src_mod=src_mod)

    def embed_generic(self, pfx, c, inputs_embeds_f32, nseq, L):
        """BertEmbeddings on caller-supplied inputs_embeds (xbert.py:199-219), inference only."""
        return self._embed(2, pfx, c, nseq, L, False, self._next_salt(), pv_x=inputs_embeds_f32)[0]

    def _embed_ln_bwd(self, pfx, c, tape, dY):
        P = self.P
        dz = self._new(*dY.shape)
        ops.ln_bwd(dY, tape.z, tape.mean, tape.rstd, P.w(pfx + "embeddings.LayerNorm.weight"), dz,
                   dgamma=P.g(pfx + "embeddings.LayerNorm.weight"), dbeta=P.g(pfx + "embeddings.LayerNorm.bias"),
                   dropout_p=self._p_hidden(c), seed=self.seed, salt=tape.salt, drop_on_dy=True)
        return dz

    # ------------------------------------------------------------------------------------------------- heads
    def _transform_fwd(self, dense, norm, X, save, *, eps, r32=False, pre=True):
        """Transform head: Linear, erf-GELU, LayerNorm (BertPredictionHeadTransform xbert.py:662-676; property_mtr_head[0:3] SPMM_models.py:
        39-42) as one GEMM with the GELU epilogue and one row kernel.  save: keep the LayerNorm's tape; pre: keep the pre-activation (the
        GELU's backward reads it); r32 (fp32 residual stream): y is the fp32 twin the loss head reads.  -> (y, HeadTape)"""
        P, M, H = self.P, X.shape[0], X.shape[1]
        t = self._new(M, H)
        pre = self._new(M, H) if pre else None
        ops.gemm_nt(X, P.wb(dense + ".weight"), t, bias=P.w(dense + ".bias"), epi=ops.EPI_GELU, C2=pre)
        y = self._new(M, H)
        mean, rstd = self._stats(M, save)
        z = t if save else None                           # (the row kernel writes the sum over its own input)
        kw = dict(zout=z, mean=mean, rstd=rstd, eps=eps)
        if r32:
            y32 = self._new(M, H, dtype=torch.float32)
            ops.ln_fwd_r32(t, None, P.w(norm + ".weight"), P.w(norm + ".bias"), y, y32=y32, **kw)
            y = y32
        else:
            ops.ln_fwd(t, None, P.w(norm + ".weight"), P.w(norm + ".bias"), y, **kw)
        return y, HeadTape(dense, norm, X, pre, LnTape(z, y, mean, rstd))

    def _transform_bwd(self, tape, dy):
        """Backward of `_transform_fwd` up to the pre-activation: -> dpre.  LayerNorm and dense-layer gradients are accumulated; the
        data-gradient GEMM on dpre stays with the caller."""
        P, ln = self.P, tape.ln
        dz = self._new(*dy.shape)
        ops.ln_bwd(dy, ln.z, ln.mean, ln.rstd, P.w(tape.norm + ".weight"), dz, dgamma=P.g(tape.norm + ".weight"), dbeta=P.g(tape.norm + ".bias"))
        dpre = self._gelu_bwd(dz, tape.pre)
        self._wgrad(dpre, tape.X, P.g(tape.dense + ".weight"), P.g(tape.dense + ".bias"))
        return dpre

    def lm_head_fwd(self, pfx, c, X, save):
        """BertOnlyMLMHead xbert.py:662-706 -> (fp32 logits [M, V], HeadTape)."""
        P = self.P
        tf = pfx + "cls.predictions.transform."
        y, tape = self._transform_fwd(tf + "dense", tf + "LayerNorm", X, save, eps=c.layer_norm_eps)
        logits = self._new(X.shape[0], c.vocab_size, dtype=torch.float32)
        ops.gemm_nt(y, P.wb(pfx + "cls.predictions.decoder.weight"), logits, bias=P.w(pfx + "cls.predictions.bias"), epi=ops.EPI_F32)
        return logits, tape

    def lm_head_bwd(self, pfx, c, tape, dlogits, out=None):
        """dlogits bf16 [M, Vpad] (zero padded) -> dX bf16 [M,H]; the decoder is tied to the word embeddings."""
        P, H, V, M = self.P, c.hidden_size, c.vocab_size, dlogits.shape[0]
        Vp = dlogits.shape[1]
        # wgrad of the tied decoder: dWord[V,H] += dlogits^T y ; dbias += colsum
        # (inline: the tied word-embedding gradient is also written by embed_bwd's atomics on the compute stream)
        self._wgrad(dlogits[:, :V], tape.ln.y, P.g(pfx + "bert.embeddings.word_embeddings.weight"), P.g(pfx + "cls.predictions.bias"), inline=True)
        dy = self._new(M, H)
        ops.gemm_nt(dlogits, P.wT_padded(pfx + "cls.decoderT", pfx + "bert.embeddings.word_embeddings.weight", Vp), dy)
        dpre = self._transform_bwd(tape, dy)
        dX = self._new(M, H) if out is None else out
        ops.gemm_nt(dpre, self._wT(pfx + "cls.transform", P.w(pfx + "cls.predictions.transform.dense.weight")), dX)
        return dX

    def _gelu_bwd(self, dz, pre):
        """elementwise dz * gelu'(pre) (small head tensors only)."""
        return ops.gelu_bwd(dz, pre)

    # ---------------------------------------------------------------------------------------------- features
    def _feat_fwd(self, proj, X, L, B, save, cls_rows=None, X32=None):
        """normalize(proj(X[:, 0, :])) SPMM_models.py:92,95,101,105 -> (feat f32 [B,E], tape).  cls_rows (int64 [B]): rows of
        the first token of every sequence when X is packed.  X32 (fp32 residual stream): the projection reads the fp32 rows with
        fp32 weights (spmm_rows_linear) instead of the bf16 MFMA GEMM."""
        P, E, H = self.P, self.cfg.embed_dim, self.cfg.text.hidden_size
        if cls_rows is not None:
            cls = X.index_select(0, cls_rows)
        else:
            cls = X.view(-1, L * H)[:B, :H]                 # strided CLS rows, row stride L*H
        raw = self._new(B, E, dtype=torch.float32)
        if X32 is not None:
            cls32 = X32.index_select(0, cls_rows) if cls_rows is not None else X32.view(-1, L * H)[:B, :H]
            ops.rows_linear(cls32, P.w(proj + ".weight"), P.w(proj + ".bias"), raw)
        else:
            ops.gemm_nt(cls, P.wb(proj + ".weight"), raw, bias=P.w(proj + ".bias"), epi=ops.EPI_F32)
        feat = self._new(B, E, dtype=torch.float32)
        nrm = self._new(B, dtype=torch.float32)
        return raw, feat, nrm, cls

    # ------------------------------------------------------------------------------------------------- banks
    def _banks(self, B):
        """bf16 GEMM shadows of the two feature banks [feat_m^T | queue] (SPMM_models.py:102,106)."""
        if self._bank is not None and self._bank["B"] == B:
            return self._bank
        E, Q = self.cfg.embed_dim, self.cfg.queue_size
        J = B + Q
        Jp = _ceil(J, 64)
        bank = {"B": B, "J": J, "Jp": Jp}
        for nm in ("prop", "text"):
            w3 = torch.zeros(J, 3 * E, dtype=BF, device=self.dev)
            qT = torch.zeros(E, Jp, dtype=BF, device=self.dev)
            ops.queue_shadow(self.P.buffers[nm + "_queue"], w3, qT, Bloc=B)
            bank[nm] = (w3, qT)
        self._bank = bank
        return bank

    def invalidate_banks(self):
        self._bank = None
