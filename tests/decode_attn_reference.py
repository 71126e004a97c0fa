"""Reference, buffers, case lists and a model of the kernels' walk for the single-query decode attention (spmm_amd/csrc/decode.hip:
spmm_decode_attn, spmm_decode_xattn -- the grouped kernel decode_attn_mfma_kernel<G, ALLSAME, VARLEN>, the one-wave-per-row kernel
decode_attn_kernel and cache_write_kernel):

    out[r, h] = sum_j softmax_j(q[r, h] . K[s(r, j), j, h] * scale) V[s(r, j), j, h]            j < L(r), head dim 64

Plain torch on the CPU; tests/test_decode_attn_edges_gpu.py runs the kernels on these cases and tests/test_decode_attn_reference_cpu.py
checks this module itself.

A Problem names one launch.  world(p) builds its data from a fixed seed; operand_buffers(p) lays them out as the launch finds them: the
key / value buffer holds NaN in EVERY cell the reference does not read (positions past the valid ones, cache rows no ancestry entry names
at that position, padding columns, rows between and after packed sources, and -- with knew / vnew -- the cells the launch itself has to
fill), ancestry entries of positions past the end name a cache row that is NaN throughout, q / knew / vnew carry NaN padding columns and
out is a view of a wider, taller buffer full of a sentinel.

reference(p) is the formula in float64 (ref64), in float32 (ref32) and A = sum_j softmax_j |v_j|.  check_output() asserts, on the whole
buffers copied back after a launch: out is finite; nothing outside the out view changed, and the key / value buffer equals its input with
exactly the new 128-byte rows at (rowmap[r], L - 1) set when knew / vnew are given; and, element by element,

    |got - ref64| <= 2^-8 (A + |ref64|) (1 + 2^-7) + f32_bound(ref64, ref32)

The first term is derived: both kernels round every probability to bf16 (unit roundoff 2^-8) in front of V -- at most 2^-8 A -- and the
output to bf16 (2^-8 |ref64| to first order; the factor 1 + 2^-7 pays for rounding the perturbed value, not the exact one); everything
else is fp32 arithmetic over exact bf16 products, which helpers_gpu.f32_bound covers (max(8 E32, 4 ulp), E32 the error of ref32).
Nothing in the bound comes from what a kernel gives.

Key-identity problems (ident=True) pin the map (beam, position) -> cache row -> output row exactly: row r's query is 16 x the key row of
one chosen position, which gives that key a float64 weight >= 1 - 2^-30 (asserted from the reference alone), its bf16 probability is
exactly 1, every other key contributes < 1e-25, and the output must be the stored bf16 value row within 2^-20 |x|.

model(p, defect) walks the keys as the kernels do (virtual keys in blocks of 16 with an online softmax and bf16 probabilities, or one
two-pass softmax per row; the newest-position copy) on the physical buffers; seven known defects can be switched on.  The CPU test asserts
that the clean model passes check_output on every case and that every defect is rejected -- the argument that the GPU tests cannot pass a
subtly wrong kernel."""
import functools
import math
import zlib
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple

import torch

from helpers_gpu import f32_bound

BF = torch.bfloat16
SENTINEL = -1234.5
PAD_ROWS, PAD_COLS = 3, 8
NAN = float("nan")
SCALE = 0.125
DEFECTS = ("last_key_dropped", "tail_to_next_beam", "s_shared", "no_rescale", "newest_from_cache", "rowmap_ignored", "t_ptr_ignored")


@dataclass(frozen=True)
class Problem:
    form: str                               # same (anc None, kv_div == group) | anc | varlen (spmm_decode_xattn) | per_row (group > 8 or kv_div != group)
    G: int                                  # `group`
    nmol: int = 2                           # R = nmol * G rows
    nH: int = 2
    Lkv: int = 37                           # the host argument (Lkv_max of spmm_decode_xattn)
    Lmax: Optional[int] = None              # positions a cache row holds (default: Lkv + 3)
    s: Optional[int] = None                 # ancestry table: the beams of a molecule share their rows below position s (None: everywhere)
    table: str = "tail"                     # "tail": own rows from s on | "random": unrelated rows of the whole cache at every position
    layout: str = "tok"                     # tok (token-major) | head (head-major) | wide (head_stride 72) | fused (K|V side by side in one row)
    t: Optional[int] = None                 # *t_ptr (None: no device-side position)
    new: bool = False                       # knew / vnew
    rowmap: bool = False                    # scattered, out-of-order cache rows in a cache larger than R
    seq0: bool = False                      # seq_stride = 0: every molecule reads sequence 0
    kv_div: Optional[int] = None            # per_row without a table
    lens: Optional[Tuple[int, ...]] = None  # varlen: kv_len of every source
    kv_seq: Optional[Tuple[int, ...]] = None
    score: str = "rand"                     # rand | equal | hot_first | hot_last | hot_tail | zero_q
    ident: bool = False                     # key-identity problem

    def __post_init__(self):
        assert self.form in ("same", "anc", "varlen", "per_row") and self.layout in ("tok", "head", "wide", "fused")
        assert self.form != "varlen" or (self.lens and self.layout == "fused" and not (self.new or self.rowmap or self.seq0 or self.t is not None))
        assert not self.new or self.has_table
        assert self.form != "per_row" or self.G > 8 or (self.kv_div and self.kv_div != self.G)
        assert self.form == "per_row" or 1 <= self.G <= 8

    @property
    def has_table(self):
        return self.form == "anc" or (self.form == "per_row" and self.kv_div is None)

    @property
    def R(self):
        return self.nmol * self.G

    @property
    def H(self):
        return self.nH * 64

    @property
    def Leff(self):                         # valid positions of a cache row
        return self.Lkv if self.t is None else min(self.t + 1, self.Lkv)

    @property
    def lmax(self):
        return self.Lmax if self.Lmax is not None else (max(self.lens) if self.lens else self.Lkv + 3)

    @property
    def ldq(self):                          # with knew / vnew: q | knew | vnew are the three column blocks of one projection output
        return (3 if self.new else 1) * self.H + PAD_COLS

    @property
    def ldo(self):
        return self.H + PAD_COLS

    @property
    def name(self):
        f = [f"{self.form}-G{self.G}-m{self.nmol}h{self.nH}-L{self.Lkv}of{self.lmax}"]
        f += [f"s{self.s}"] if self.s is not None else []
        f += [self.table] if self.table != "tail" else []
        f += [self.layout] if self.layout != "tok" else []
        f += [f"t{self.t}"] if self.t is not None else []
        f += [n for n, on in (("new", self.new), ("rowmap", self.rowmap), ("seq0", self.seq0), ("ident", self.ident)) if on]
        f += [f"div{self.kv_div}"] if self.kv_div else []
        f += ["len" + ".".join(map(str, self.lens))] if self.lens else []
        f += ["seq" + ("".join(map(str, self.kv_seq)) if len(self.kv_seq) <= 8 else f"x{len(self.kv_seq)}")] if self.kv_seq else []
        f += [self.score] if self.score != "rand" else []
        return "-".join(f)


def _gen(p, salt):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(f"{p.name}/{salt}".encode()))


def _randn(p, salt, *shape):
    return torch.randn(*shape, generator=_gen(p, salt)).to(BF)


def _pm(p, salt, *shape):
    """+-[0.25, 2] rounded to bf16 (the rounding keeps the range)."""
    g = _gen(p, salt)
    mag = 0.25 + 1.75 * torch.rand(*shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return (mag * sign).to(BF)


# ---------------------------------------------------------------------------------------------------------------------
# the data of a problem
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(p):
    """Everything problem p is made of, in logical form (shared, never modified):
      q [R, nH, 64], knew / vnew [R, nH, 64] or None (bf16)
      Kb, Vb [S, lmax, nH, 64] finite bf16 for every cell of the cache; named [S, lmax]: the cells the reference reads from the cache
      src [R, lmax] (long): the cache row (source, for varlen) of position j of row r; lens [R]: valid positions of row r
      own [R]: the cache row row r's newest position belongs to; dead: a cache row that is NaN throughout
      anc [R, anc_ld] int32 or None; geometry: seq_off [S], tok, hs, koff, voff, total (elements of the flat key / value buffer)
      hot [R, nH] (long) or None: the position whose key the query was built from (ident and hot_* scores)."""
    R, G, nH, H, L, lmax = p.R, p.G, p.nH, p.H, p.Leff, p.lmax
    w = SimpleNamespace(p=p, anc=None, hot=None, knew=None, vnew=None, row0=None, kv_len=None)
    ar = torch.arange(R)
    # ---- which cache row holds position j of row r
    if p.form == "varlen":
        U = len(p.lens)
        seq = torch.tensor(p.kv_seq if p.kv_seq is not None else list(range(p.nmol)))
        assert len(seq) == p.nmol and int(seq.max()) < U
        S, w.dead = U, None
        w.src = seq.repeat_interleave(G)[:, None].expand(R, lmax).contiguous()
        w.lens = torch.tensor([min(max(p.lens[u], 1), p.Lkv) for u in seq.tolist()]).repeat_interleave(G)
        w.own = ar
    elif not p.has_table:
        div = p.G if p.form == "same" else p.kv_div
        S = 1 if p.seq0 else -(-R // div) + 1
        w.dead = None if p.seq0 else S - 1
        w.src = (torch.zeros(R, dtype=torch.long) if p.seq0 else ar // div)[:, None].expand(R, lmax).contiguous()
        w.lens = torch.full((R,), L)
        w.own = ar
    else:
        S = (2 * R + 3) if p.rowmap else R + 1
        w.dead = S - 1
        w.own = torch.randperm(S - 1, generator=_gen(p, "rowmap"))[:R] if p.rowmap else ar
        if p.rowmap and w.own.tolist() == sorted(w.own.tolist()):
            w.own = w.own.flip(0)                                                # (out of order, whatever the draw)
        mol, beam = ar // G, ar % G
        own_of = lambda m, b: w.own[m * G + b]
        s = L if p.s is None else p.s
        assert 0 <= s <= L
        w.src = torch.full((R, lmax), w.dead)
        for j in range(L):
            if p.table == "random" and not (p.new and j == L - 1):
                w.src[:, j] = torch.randint(0, S - 1, (R,), generator=_gen(p, f"anc{j}"))
            elif j < s and not (p.new and j == L - 1):
                w.src[:, j] = own_of(mol, torch.full_like(mol, j % G))           # inherited from one parent: the same row for every beam
            else:
                w.src[:, j] = own_of(mol, (beam + (L - 1 - j)) % G)              # rows of the molecule's own beams; the newest is the row's own
        w.lens = torch.full((R,), L)
        anc_ld = lmax + 3
        w.anc = torch.full((R, anc_ld), w.dead, dtype=torch.int32)
        w.anc[:, :lmax] = w.src.to(torch.int32)
    w.S = S
    pos = torch.arange(lmax)
    live = pos[None, :] < w.lens[:, None]                                        # [R, lmax]
    w.named = torch.zeros(S, lmax, dtype=torch.bool)
    w.named[w.src[live], pos[None, :].expand(R, lmax)[live]] = True
    if p.new:
        w.named[w.own, L - 1] = False                                            # the launch fills these
        assert not w.named[:, L - 1].any()
    assert w.dead is None or not w.named[w.dead].any()
    # ---- values
    w.q = _randn(p, "q", R, nH, 64)
    w.Kb = _pm(p, "K", S, lmax, nH, 64) if p.ident else _randn(p, "K", S, lmax, nH, 64)     # (ident: |k|^2 far above any k . k')
    w.Vb = _pm(p, "V", S, lmax, nH, 64) if p.ident else _randn(p, "V", S, lmax, nH, 64)
    if p.new:
        w.knew = _pm(p, "knew", R, nH, 64) if p.ident else _randn(p, "knew", R, nH, 64)
        w.vnew = _pm(p, "vnew", R, nH, 64) if p.ident else _randn(p, "vnew", R, nH, 64)
    if p.score == "equal":
        w.Kb = w.Kb[:1, :1, :1].expand(S, lmax, nH, 64).contiguous()
        if p.new:
            w.knew = w.Kb[0, 0, 0].expand(R, nH, 64).contiguous()
    elif p.score == "zero_q":
        w.q = torch.zeros_like(w.q)
    hot_scale = None
    if p.ident:
        # rows of one molecule sit on different positions, molecules shift them: every (beam, position) is some row's hot key
        idx = (ar // G) if p.form != "varlen" else _rank_in_source(w.src[::G, 0]).repeat_interleave(G)
        w.hot = ((idx + ar % G)[:, None] + torch.arange(nH)[None, :]) % w.lens[:, None]
        hot_scale = 16.0
    elif p.score.startswith("hot_"):
        tail = (L if p.s is None else p.s) if p.has_table else L - 2
        j = {"hot_first": min(3, L - 1), "hot_last": L - 1, "hot_tail": max(min(tail, L - 1), 0)}[p.score]
        w.hot = torch.full((R, nH), j)
        hot_scale = 32.0
    if hot_scale is not None:
        hh = torch.arange(nH)[None, :].expand(R, nH)
        rows = w.src[ar[:, None], w.hot]                                        # [R, nH]
        from_new = (w.hot == (w.lens[:, None] - 1)) & p.new
        if p.ident:
            key = torch.where(from_new[..., None], w.knew if p.new else w.Kb[rows, w.hot, hh], w.Kb[rows, w.hot, hh])
            w.q = (key.float() * hot_scale).to(BF)
        else:
            # the key becomes 32 x the query of the LAST row that names it (a shared key: one beam's query; the others see a large score of either sign)
            for r in range(R):
                for h in range(nH):
                    k = (w.q[r, h].float() * hot_scale).to(BF)
                    if from_new[r, h]:
                        w.knew[r, h] = k
                    else:
                        w.Kb[rows[r, h], w.hot[r, h], h] = k
    # ---- geometry of the flat key / value buffer: element (s, j, h, d) of K at koff + seq_off[s] + j * tok + h * hs + d, of V at voff + ...
    if p.form == "varlen":
        gap, row0, at = 2, [], 1
        for n in p.lens:
            row0.append(at)
            at += n + gap
        w.row0, w.kv_len = torch.tensor(row0, dtype=torch.int32), torch.tensor(p.lens, dtype=torch.int32)
        w.tok, w.hs, w.koff, w.voff = 2 * H + 8, 64, 0, H
        w.seq_stride, w.seq_off, w.total = 0, w.row0.long() * w.tok, at * w.tok
    else:
        if p.layout == "tok":
            w.tok, w.hs = H + 8, 64
            seq = lmax * w.tok + 16
        elif p.layout == "wide":
            w.tok, w.hs = nH * 72 + 8, 72
            seq = lmax * w.tok
        elif p.layout == "head":
            w.tok, w.hs = 64, lmax * 64
            seq = nH * w.hs + 8
        else:
            w.tok, w.hs = 2 * H + 8, 64
            seq = lmax * w.tok
        region = S * seq
        w.koff, w.voff, w.total = (0, H, region + 8) if p.layout == "fused" else (0, region + 8, 2 * region + 16)
        w.seq_stride = 0 if p.seq0 else seq
        w.seq_off = torch.arange(S) * w.seq_stride
    assert all(x % 8 == 0 for x in (w.tok, w.hs, w.koff, w.voff, w.seq_stride, w.total)) and 255 * w.tok < 2 ** 31
    return w


def _rank_in_source(seq):
    """seq [n] -> how many earlier entries name the same source."""
    seen, out = {}, []
    for u in seq.tolist():
        out.append(seen.get(u, 0))
        seen[u] = out[-1] + 1
    return torch.tensor(out)


def cell_index(w, s, j):
    """Flat element indices, relative to K's / V's first element, of the 128-byte rows of the cells (s[i], j[i]) -> [n, nH, 64]."""
    h, d = torch.arange(w.p.nH), torch.arange(64)
    return (w.seq_off[s] + j * w.tok)[:, None, None] + (h * w.hs)[None, :, None] + d[None, None, :]


def operand_buffers(p):
    """The buffers of problem p as the launch finds them (fresh CPU tensors):
      qkv [R, ldq] bf16: q = [:, :H] (with knew / vnew: knew = [:, H:2H], vnew = [:, 2H:3H]), NaN in the padding columns
      kv  [total] bf16: the flat key / value buffer, NaN in every cell the reference does not read
      out [R + PAD_ROWS, ldo] bf16 full of SENTINEL: the launch writes the view [:R, :H]
      anc int32 [R, lmax + 3] or None; t int32 [1] or None; rowmap int32 [R] or None; row0, kv_len, kv_seq int32 or None."""
    w = world(p)
    qkv = torch.full((p.R, p.ldq), NAN, dtype=BF)
    qkv[:, :p.H] = w.q.reshape(p.R, p.H)
    if p.new:
        qkv[:, p.H:2 * p.H] = w.knew.reshape(p.R, p.H)
        qkv[:, 2 * p.H:3 * p.H] = w.vnew.reshape(p.R, p.H)
    kv = torch.full((w.total,), NAN, dtype=BF)
    s, j = w.named.nonzero(as_tuple=True)
    idx = cell_index(w, s, j)
    kv[w.koff + idx] = w.Kb[s, j]
    kv[w.voff + idx] = w.Vb[s, j]
    return SimpleNamespace(qkv=qkv, kv=kv, out=torch.full((p.R + PAD_ROWS, p.ldo), SENTINEL, dtype=BF),
                           anc=None if w.anc is None else w.anc.clone(),
                           t=None if p.t is None else torch.tensor([p.t], dtype=torch.int32),
                           rowmap=w.own.to(torch.int32) if p.rowmap else None,
                           row0=w.row0, kv_len=w.kv_len, kv_seq=None if p.kv_seq is None else torch.tensor(p.kv_seq, dtype=torch.int32))


def launch_spec(p):
    """The scalar arguments of the launch: strides in elements, the offsets of K and V in the flat buffer, kv_div."""
    w = world(p)
    kv_div = 1 if p.has_table else (p.G if p.form in ("same", "varlen") else p.kv_div)
    return SimpleNamespace(seq_stride=int(w.seq_stride), tok=w.tok, hs=w.hs, koff=w.koff, voff=w.voff, kv_div=kv_div, anc_ld=None if w.anc is None else w.anc.shape[1])


def score_lead(p):
    """[R, nH] float64: the largest score of every (row, head) minus its second largest (inf with one key)."""
    K, _, live = gathered(p)
    sc = torch.einsum("rhd,rjhd->rhj", world(p).q.double(), K.double()) * SCALE
    sc = sc.masked_fill(~live[:, None, :], -math.inf)
    top = sc.topk(min(2, sc.shape[-1]), -1).values
    return top[..., 0] - top[..., 1] if top.shape[-1] > 1 else torch.full(top.shape[:2], math.inf, dtype=torch.float64)


def applicable_defects(p):
    """The defects of model() that MUST change what check_output sees of problem p (a condition on the problem, not a measurement)."""
    grouped_tail = p.form == "anc" and p.G > 1 and any(s < p.Leff for s, _ in parting(p))
    out = [] if p.score in ("hot_first", "hot_tail") else ["last_key_dropped"]           # (a key that far behind weighs nothing)
    out += ["tail_to_next_beam"] if grouped_tail and p.score != "hot_first" else []          # (the tail weighs nothing behind a hot shared key ...
    out += ["s_shared"] if grouped_tail and p.score not in ("hot_first", "hot_last") else []  #  ... and position s nothing behind a hot later one)
    # without the rescale a wave is wrong as soon as its maximum rises after the first block: certain where the hot key sits in a later block
    out += ["no_rescale"] if is_grouped(p) and (p.score in ("hot_last", "hot_tail") or p.ident) and max(nv for _, nv in parting(p)) > 16 else []
    out += ["newest_from_cache"] if p.new else []
    out += ["rowmap_ignored"] if p.new and p.rowmap else []
    out += ["t_ptr_ignored"] if p.t is not None and p.t + 1 < p.Lkv else []
    return out


def expected_kv(p):
    """The flat key / value buffer after the launch: the input, with the new rows at (own[r], Leff - 1) when knew / vnew are given."""
    w, kv = world(p), operand_buffers(p).kv
    if p.new:
        idx = cell_index(w, w.own, torch.full((p.R,), p.Leff - 1))
        kv[w.koff + idx] = w.knew
        kv[w.voff + idx] = w.vnew
    return kv


def gathered(p):
    """(K, V) [R, Lg, nH, 64] bf16 as the reference reads them (the newest position from knew / vnew), live [R, Lg]."""
    w = world(p)
    Lg = int(w.lens.max())
    pos = torch.arange(Lg)
    K, V = w.Kb[w.src[:, :Lg], pos[None, :]].clone(), w.Vb[w.src[:, :Lg], pos[None, :]].clone()
    if p.new:
        K[:, p.Leff - 1], V[:, p.Leff - 1] = w.knew, w.vnew
    return K, V, pos[None, :] < w.lens[:, None]


def attention(q, K, V, live, dtype):
    """softmax_j(q . K_j * SCALE) V_j with every operation in dtype: q [R, nH, 64], K / V [R, L, nH, 64], live [R, L] -> (out, A, P)."""
    sc = torch.einsum("rhd,rjhd->rhj", q.to(dtype), K.to(dtype)) * SCALE
    sc = sc.masked_fill(~live[:, None, :], -math.inf)
    P = torch.softmax(sc, -1)
    return torch.einsum("rhj,rjhd->rhd", P, V.to(dtype)), torch.einsum("rhj,rjhd->rhd", P, V.to(dtype).abs()), P


@functools.lru_cache(maxsize=None)
def reference(p):
    """(ref64, A, ref32) [R, nH * 64]: computed once per problem, shared, never modified.  Key-identity problems assert their premise here."""
    w = world(p)
    K, V, live = gathered(p)
    ref64, A, P = attention(w.q, K, V, live, torch.float64)
    ref32 = attention(w.q, K, V, live, torch.float32)[0]
    if p.ident:
        weight = P.gather(2, w.hot[:, :, None])[..., 0]
        assert bool((weight >= 1 - 2.0 ** -30).all()), f"{p.name}: hot key weight {weight.min().item()}"
        assert bool((hot_values(p).float().abs() >= 2.0 ** -6).all())
    return ref64.reshape(p.R, p.H), A.reshape(p.R, p.H), ref32.reshape(p.R, p.H)


def hot_values(p):
    """Key-identity problems: the stored bf16 value row of every row's hot key [R, nH * 64]."""
    w = world(p)
    V = gathered(p)[1]
    return V[torch.arange(p.R)[:, None], w.hot, torch.arange(p.nH)[None, :]].reshape(p.R, p.H)


def _bits(t):
    return t.contiguous().view(torch.int16)


def check_output(name, bufs, p):
    """bufs: .out and .kv after the launch, whole buffers on the CPU.  Asserts finiteness, the untouched cells and the bound (module
    docstring); prints E32, the largest error and the largest err / allow."""
    ref64, A, ref32 = reference(p)
    out, kv = bufs.out, bufs.kv
    assert out.dtype == BF and tuple(out.shape) == (p.R + PAD_ROWS, p.ldo) and kv.dtype == BF and kv.numel() == world(p).total
    view = out[:p.R, :p.H]
    finite = torch.isfinite(view.float())
    assert finite.all(), f"{name}: {int((~finite).sum())} non-finite outputs; first {(~finite).nonzero()[0].tolist()}"
    outside = torch.ones(out.shape, dtype=torch.bool)
    outside[:p.R, :p.H] = False
    touched = outside & (_bits(out) != _bits(torch.tensor([SENTINEL], dtype=BF)))
    assert not touched.any(), f"{name}: {int(touched.sum())} elements outside out[:{p.R}, :{p.H}] written; first {touched.nonzero()[0].tolist()}"
    wrong = _bits(kv) != _bits(expected_kv(p))
    assert not wrong.any(), f"{name}: {int(wrong.sum())} elements of the key / value buffer differ from input + new rows; first at {int(wrong.nonzero()[0])}"
    E32, b32 = f32_bound(ref64, ref32)
    err = (view.double() - ref64).abs()
    allow = 2.0 ** -8 * (A + ref64.abs()) * (1 + 2.0 ** -7) + b32
    margin = (err / allow).max().item()
    print(f"[tol] {name}: E32={E32:.3e} kernel={err.max().item():.3e} margin={margin:.3f}")
    ok = err <= allow
    assert ok.all(), f"{name}: {int((~ok).sum())}/{ok.numel()} past the bound; max err {err.max().item():.4g}, err/allow {margin:.3f}, " \
                     f"first bad {(~ok).nonzero()[0].tolist()}"
    if p.ident:
        x = hot_values(p).double()
        off = (view.double() - x).abs() > 2.0 ** -20 * x.abs()
        assert not off.any(), f"{name}: {int(off.sum())} elements are not the hot key's value; first {off.nonzero()[0].tolist()} " \
                              f"(rows {sorted(set(off.nonzero()[:, 0].tolist()))[:8]})"


# ---------------------------------------------------------------------------------------------------------------------
# what the kernels derive from a problem
# ---------------------------------------------------------------------------------------------------------------------
def is_grouped(p):
    return p.form != "per_row"


def parting(p, L=None, extra=0):
    """Grouped kernel: per molecule, (s, nv) as the kernel derives them from the table: s = the first position < L where some beam's
    entry differs from beam 0's (L when none; at most L - 1 with knew / vnew), nv = s + G (L - s).  same / varlen: s = nv = L."""
    w = world(p)
    out = []
    for n in range(p.nmol):
        Ln = int(w.lens[n * p.G]) if L is None else L
        s = Ln
        if p.form == "anc":
            t = w.anc[n * p.G:(n + 1) * p.G, :Ln]
            diff = (t != t[:1]).any(0).nonzero()
            s = int(diff[0]) if len(diff) else Ln
            if p.new:
                s = min(s, Ln - 1)
            s = min(s + extra, Ln)
        out.append((s, s + p.G * (Ln - s)))
    return out


def _f(x):
    return x.float()


def model(p, defect=None):
    """The buffers (.out, .kv) as the kernels' walk leaves them, read from and written to the physical buffers of operand_buffers(p);
    defect: one of DEFECTS.
      last_key_dropped    the last (virtual) key is masked            tail_to_next_beam   per-beam keys are shown to beam (b + 1) % G
      s_shared            position s is read as a shared one          no_rescale          the accumulators keep their scale at a new maximum
      newest_from_cache   position L - 1 comes from the cache, not from knew / vnew (per row: the copy launch is missing)
      rowmap_ignored      the copy writes to cache row r              t_ptr_ignored       the host's Lkv is used"""
    assert defect is None or defect in DEFECTS
    w, b = world(p), operand_buffers(p)
    R, G, nH, H = p.R, p.G, p.nH, p.H
    kv = b.kv
    L = p.Lkv if (defect == "t_ptr_ignored" or p.t is None) else min(p.t + 1, p.Lkv)
    q = b.qkv[:, :H].reshape(R, nH, 64)
    if p.new:
        knew, vnew = b.qkv[:, H:2 * H].reshape(R, nH, 64), b.qkv[:, 2 * H:3 * H].reshape(R, nH, 64)
        dst = torch.arange(R) if defect == "rowmap_ignored" or b.rowmap is None else b.rowmap.long()
        idx = cell_index(w, dst, torch.full((R,), L - 1))
        after = kv.clone()
        after[w.koff + idx], after[w.voff + idx] = knew, vnew
    else:
        after = kv
    out = b.out
    if not is_grouped(p):
        # ---- decode_attn_kernel: one row at a time, the cache as cache_write_kernel left it, two passes
        read = kv if (p.new and defect == "newest_from_cache") else after
        pos = torch.arange(L)
        rows = b.anc[:, :L].long() if b.anc is not None else (torch.arange(R) // p.kv_div)[:, None].expand(R, L)
        idx = cell_index(w, rows.reshape(-1), pos.repeat(R)).reshape(R, L, nH, 64)
        K, V = _f(read[w.koff + idx]), _f(read[w.voff + idx])
        sc = torch.einsum("rhd,rjhd->rhj", _f(q) * SCALE, K)
        if defect == "last_key_dropped":
            sc[:, :, L - 1] = -math.inf
        e = torch.exp(sc - sc.max(-1, keepdim=True).values)
        e = torch.where(torch.isneginf(sc), torch.zeros_like(e), e)
        o = torch.einsum("rhj,rjhd->rhd", _f(e.to(BF)), V) / e.sum(-1)[..., None]
        out[:R, :H] = o.to(BF).reshape(R, H)
        return SimpleNamespace(out=out, kv=after)
    # ---- decode_attn_mfma_kernel: one wave per (molecule, head); virtual keys in blocks of 16, online softmax
    nmol = p.nmol
    if p.form == "varlen":
        Ls = [int(w.lens[n * G]) for n in range(nmol)]
        sn = [(l, l) for l in Ls]
    else:
        Ls = [L] * nmol
        sn = parting(p, L, extra=1 if defect == "s_shared" else 0) if p.form == "anc" else [(L, L)] * nmol
    NV = -(-max(nv for _, nv in sn) // 16) * 16
    v = torch.arange(NV)
    Kk, Vk = torch.zeros(nmol, NV, nH, 64), torch.zeros(nmol, NV, nH, 64)
    vis = torch.zeros(nmol, NV, G, dtype=torch.bool)
    for n, (s, nv) in enumerate(sn):
        vc = v.clamp(max=nv - 1)                                                 # keys past the end re-read the last one
        tail = vc >= s
        j = torch.where(tail, s + (vc - s) // G, vc)
        bm = torch.where(tail, (vc - s) % G, torch.zeros_like(vc))
        if p.form == "anc":
            rows = b.anc[n * G + bm, j].long()
        elif p.form == "varlen":
            rows = torch.full((NV,), int(w.src[n * G, 0]))
        else:
            rows = torch.zeros(NV, dtype=torch.long) if p.seq0 else torch.full((NV,), (n * G) // G)
        idx = cell_index(w, rows, j)
        Kn, Vn = _f(kv[w.koff + idx]), _f(kv[w.voff + idx])
        if p.new and defect != "newest_from_cache":
            newest = tail & (j == Ls[n] - 1)
            Kn[newest], Vn[newest] = _f(knew[n * G + bm[newest]]), _f(vnew[n * G + bm[newest]])
        Kk[n], Vk[n] = Kn, Vn
        ok = v < (nv - 1 if defect == "last_key_dropped" else nv)
        beams = torch.arange(G)[None, :]
        mine = (((bm + 1) % G) if defect == "tail_to_next_beam" else bm)[:, None] == beams
        vis[n] = ok[:, None] & (~(v >= s)[:, None] | mine)
    qm = _f(q).reshape(nmol, G, nH, 64)
    sc = torch.einsum("nvhd,nghd->nhvg", Kk, qm) * SCALE                         # [nmol, nH, NV, G]
    sc = torch.where(vis[:, None], sc, torch.full_like(sc, -math.inf))
    mrun = torch.full((nmol, nH, G), -math.inf)
    lrun = torch.zeros(nmol, nH, G)
    acc = torch.zeros(nmol, nH, G, 64)
    for i in range(NV // 16):
        sv = sc[:, :, i * 16:i * 16 + 16]
        mn = torch.maximum(mrun, sv.max(2).values)
        mu = torch.where(torch.isneginf(mn), torch.zeros_like(mn), mn)
        alpha = torch.ones_like(mu) if (defect == "no_rescale" and i > 0) else torch.exp(mrun - mu)
        mrun = mn
        ev = torch.exp(sv - mu[:, :, None, :])
        lrun = lrun * alpha + ev.sum(2)
        acc = acc * alpha[..., None] + torch.einsum("nhvg,nvhd->nhgd", _f(ev.to(BF)), Vk[:, i * 16:i * 16 + 16])
    o = (acc / lrun[..., None]).permute(0, 2, 1, 3)                              # [nmol, G, nH, 64]
    out[:R, :H] = o.to(BF).reshape(R, H)
    return SimpleNamespace(out=out, kv=after)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_decode_attn_edges_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
P = Problem
GS = tuple(range(1, 9))
NV_SET = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49)
S_EDGES = (0, 15, 16, 17, 31, 32)                        # with Lkv = 40: plus s = Lkv - 1 and s = Lkv (no table entry differs)
LKV_SET = (1, 63, 64, 65, 128, 129, 192, 193, 255, 256)

# a. every instantiation: G = 1..8 x {shared rows, ancestry table, variable-length memory}, 3 molecules x 2 heads, 37 keys (3 blocks when shared)
CASES_INSTANTIATIONS = ([P("same", G, nmol=3) for G in GS] + [P("anc", G, nmol=3, s=31) for G in GS]
                        + [P("varlen", G, nmol=3, lens=(37, 20, 33), layout="fused") for G in GS])

# b. where ancestries part: a block wholly shared, mixed, all per-beam; G = 3 (never launched with a table before) and G = 5 (the product's)
CASES_PARTING = [P("anc", G, Lkv=40, s=s) for G in (3, 5) for s in S_EDGES + (39, None)]

# c. virtual key counts nv = s + G (Lkv - s): 1 .. 4 blocks, the `newer` waits and the odd last round.  nv = 17 at G = 4, 33 at G = 7 / 8 and
#    49 at G = 3 leave ONE key in the last block: beam G - 1's (the walk ends on the last beam), so that block is empty for every other beam;
#    at G = 1 and 17 keys that lone key is beam 0's, and the block is empty for the 15 idle columns of the MFMA tile
NV_TABLE = [(1, 1, None, 1), (1, 17, None, 17), (2, 14, 13, 15), (3, 12, 10, 16), (4, 11, 9, 17), (5, 23, 21, 31), (6, 22, 20, 32), (7, 21, 19, 33),
            (8, 26, 25, 33), (8, 33, 31, 47), (2, 46, 44, 48), (3, 45, 43, 49)]                  # (G, Lkv, s, nv)
CASES_NV = [P("anc", G, Lkv=L, s=s) for (G, L, s, _) in NV_TABLE] + [P("same", 4, Lkv=nv) for nv in NV_SET]

# d. Lkv: the 64-lane ancestry loads (1 .. 4 of them) and LD = (Lkv + 3) & ~3; 256 positions of 8 unrelated beams: the largest LDS (16 KiB)
CASES_LKV = ([P("anc", 2 + i % 7, Lkv=L, Lmax=max(L, 8), s=max(L - 3, 0)) for i, L in enumerate(LKV_SET)]
             + [P("anc", 8, Lkv=256, Lmax=256, table="random")])

# e. arguments with an ancestry table
CASES_T_PTR = [P("anc", 3, Lkv=256, Lmax=256, t=t1 - 1, s=max(t1 - 2, 0)) for t1 in LKV_SET] + [P("anc", 3, Lkv=40, Lmax=48, t=44, s=38)]
CASES_NEW = [P("anc", G, Lkv=L, Lmax=max(L, 4), s=max(L - 3, 0), new=True) for G in GS for L in (1, 2, 17, 256)]
CASES_NEW_ARGS = ([P("anc", 5, Lkv=32, Lmax=32, t=t, s=max(min(t + 1, 32) - 4, 0), new=True) for t in (0, 16, 31, 40)]
                  + [P("anc", G, Lkv=19, s=15, new=True, rowmap=True) for G in (1, 3, 5, 8)]
                  + [P("anc", 6, Lkv=24, Lmax=24, t=17, s=13, new=True, rowmap=True, layout="head")]
                  + [P("anc", G, Lkv=19, s=14, new=True, layout="head") for G in (2, 5)]
                  + [P("anc", 4, Lkv=19, s=14, new=True, layout="wide")])

# f. arguments with shared rows: the fused K|V buffer, seq_stride = 0 (the guided search's shared baseline memory), head_stride > 64; at the
#    G no test launched with shared rows before
CASES_SAME_ARGS = [P("same", G, Lkv=23, layout=lay, seq0=z) for G in (1, 2, 4, 7) for (lay, z) in (("fused", False), ("fused", True), ("wide", False), ("head", False))]

# g. the one-wave-per-row kernel and cache_write_kernel: group > 8 with a table, or no table and kv_div != group
CASES_PER_ROW = ([P("per_row", G, nmol=1, Lkv=21, s=17, new=new, t=t, Lmax=24) for G in (9, 12, 32) for (new, t) in ((False, None), (True, None), (False, 18), (True, 18), (True, 30))]
                 + [P("per_row", 12, nmol=1, Lkv=21, s=17, new=True, rowmap=True, layout="head")]
                 + [P("per_row", 9, nmol=1, Lkv=L, Lmax=max(L, 4), s=max(L - 2, 0), new=new) for L in (1, 7, 8, 9, 256) for new in (False, True)]
                 + [P("per_row", G, nmol=n, nH=nH, kv_div=1, Lkv=9) for (G, n, nH) in ((3, 1, 1), (2, 1, 2), (5, 1, 1))]     # R * nH = 3, 4, 5
                 + [P("per_row", 4, nmol=3, kv_div=2, Lkv=33, layout="fused"), P("per_row", 12, nmol=2, kv_div=12, Lkv=33, nH=3)])

# h. variable-length memory: lengths either side of a block, longer than Lkv_max (clamped), sources permuted and repeated, NaN rows between
CASES_VARLEN = ([P("varlen", G, nmol=5, lens=(1, 15, 16, 17, 33), Lkv=33, layout="fused") for G in (1, 3, 5, 8)]
                + [P("varlen", G, nmol=7, lens=(1, 15, 16, 17, 33), kv_seq=(4, 0, 2, 2, 1, 3, 0), Lkv=40, layout="fused") for G in (2, 6)]
                + [P("varlen", G, nmol=3, lens=(33, 5, 21), Lkv=20, layout="fused") for G in (4, 7)])

# i. grid rounding and the XCD remap: nmol * nH = 1, 7, 8, 9 waves
CASES_GRID = [P(form, 2, nmol=n, nH=nH, Lkv=18, s=s) for (n, nH) in ((1, 1), (7, 1), (4, 2), (3, 3)) for (form, s) in (("same", None), ("anc", 15))]

# j. score extremes: all scores equal, one key ahead by > 100 in the first block / the last block / the per-beam tail, queries of zeros
CASES_EXTREMES = ([P("anc", 5, Lkv=40, s=34, score=sc) for sc in ("equal", "hot_first", "hot_last", "hot_tail", "zero_q")]
                  + [P("same", 5, Lkv=40, score=sc) for sc in ("equal", "hot_first", "hot_last", "hot_tail", "zero_q")]
                  + [P("per_row", 9, nmol=1, Lkv=40, s=34, score=sc) for sc in ("equal", "hot_first", "hot_last", "hot_tail", "zero_q")]
                  + [P("anc", 3, Lkv=9, s=6, new=True, score=sc) for sc in ("equal", "hot_last")])

# k. key identity: nmol = Lkv molecules sweep every position for every beam
CASES_IDENTITY = [P("anc", 3, nmol=36, Lkv=36, s=30, ident=True),                            # prefix, position s, per-beam tail: 48 virtual keys
                  P("anc", 8, nmol=19, Lkv=19, s=17, ident=True),                            # 33 virtual keys: a lone key in the last block
                  P("anc", 5, nmol=20, Lkv=20, s=16, new=True, rowmap=True, layout="head", ident=True),
                  P("anc", 2, nmol=9, Lkv=9, table="random", new=True, ident=True),
                  P("same", 4, nmol=33, Lkv=33, layout="fused", ident=True),
                  P("same", 7, nmol=18, Lkv=18, layout="fused", seq0=True, ident=True),
                  P("varlen", 3, nmol=38, lens=(17, 5, 16), Lkv=17, layout="fused", ident=True,
                    kv_seq=tuple([0, 2, 1] * 5 + [2, 0] * 11 + [0])),
                  P("per_row", 9, nmol=21, Lkv=21, s=17, new=True, rowmap=True, ident=True),
                  P("per_row", 3, nmol=10, nH=1, kv_div=1, Lkv=10, ident=True)]

FAMILIES = {"instantiations": CASES_INSTANTIATIONS, "parting": CASES_PARTING, "nv": CASES_NV, "lkv": CASES_LKV, "t_ptr": CASES_T_PTR,
            "new": CASES_NEW, "new_args": CASES_NEW_ARGS, "same_args": CASES_SAME_ARGS, "per_row": CASES_PER_ROW, "varlen": CASES_VARLEN,
            "grid": CASES_GRID, "extremes": CASES_EXTREMES, "identity": CASES_IDENTITY}
ALL_CASES = [p for cases in FAMILIES.values() for p in cases]


def case_id(p):
    return p.name


def instantiation(p):
    """(G, ALLSAME, VARLEN) of the grouped kernel a problem launches (None: the per-row kernel)."""
    return (p.G, p.form != "anc", p.form == "varlen") if is_grouped(p) else None
