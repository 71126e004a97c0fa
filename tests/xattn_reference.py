"""Float64 reference, bf16 storage model, case tables and checker for the fused cross-attention block spmm_xattn_fwd
(spmm_amd/csrc/xattn.hip).  Plain torch / numpy on the CPU; tests/test_xattn_block_gpu.py runs the kernel on these cases and
tests/test_xattn_reference_cpu.py checks this module itself.

    ctx = dropout_a(softmax(Q K^T / 8 + finfo(float32).min * (1 - kmask))) V          xbert.py:305-354
    x   = ctx Wo^T + bo                                                               xbert.py:369-373
    z   = dropout_h(x) + R
    y   = LayerNorm(z)

xattn_ref64() evaluates that formula by formula in float64, on a launch described as ops.xattn_fwd takes it, with the dropout masks of
the host model of the counter hash (helpers_gpu.py).  storage_model=True adds the bf16 roundings of the kernel and nothing else.

The comparison (check_xattn) has no fixed tolerance.  The bf16 outputs ctx, z, y and the row statistics mean, rstd follow
helpers_gpu.check_attention_parity's rule per block -- (sequence, head) for ctx, sequence for the others:

    ||got - ref64|| <= 2 ||model - ref64|| + 2^-9 ||ref64||           model = the storage model

lse is an fp32 output that no bf16 rounding feeds: helpers_gpu.check_ref against an fp32 CPU evaluation of the same formula (xattn_lse32).
defect= of xattn_ref64 returns what a kernel with one known defect would compute; the CPU test asserts that check_xattn rejects each."""
import functools
import zlib

import numpy as np
import torch

from helpers_gpu import (_bf16, _host_dropout_keep, _ints, _worst_ratio, attention_keep_mask, attention_parity_blocks, attention_ref64,
                         check_attention_parity, check_ref, f32_bound)

BF = torch.bfloat16
GAP = 3                                      # rows between (and after) the packed sequences of a Q / R / Y tensor: no sequence owns them
SEED = 20261020
DEFECTS = ("counter_q_len", "row_plus_one", "row_base_low_word", "last_key_tile", "kv_len_unmasked", "x_unrounded_stats_from_Z",
           "residual_before_mask", "neighbour_stats")


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's arithmetic (xattn.hip, spmm_xattn_fwd: `grid`, `nt`, the XA_NT switch)
# ---------------------------------------------------------------------------------------------------------------------
def instantiation(H, Lkv):
    """(NT, NCT) of the xattn_fwd_kernel<NT, NCT> that a launch with hidden width H and dense key length Lkv runs."""
    assert H in (128, 256, 768) and 1 <= Lkv <= 128
    return min(4, (Lkv + 31) // 32), {128: 1, 256: 2, 768: 6}[H]


def panels(Lq):
    """grid.x: 64-row panels per sequence (of the launch's dense Lq; a packed sequence leaves the panels past its q_len at once)."""
    return (Lq + 63) // 64


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def seq_rows(c):
    """[(first row, rows)] of every query sequence in the launch's Q / R / Y tensors."""
    q_row0, q_len = _ints(c["q_row0"]), _ints(c["q_len"])
    return [(s * c["Lq"] if q_row0 is None else q_row0[s], c["Lq"] if q_len is None else q_len[s]) for s in range(c["nseq"])]


def xattn_ref64(Q, K, V, Wo, bo, R, gamma, beta, *, eps, nseq, nH, Lq, Lkv, kmask=None, kv_seq=None, q_row0=None, q_len=None, kv_row0=None,
                kv_len=None, attn_dropout_p=0.0, hidden_dropout_p=0.0, seed=None, salt_a=0, salt_h=0, row_base=0, storage_model=False,
                defect=None):
    """One launch of ops.xattn_fwd in float64.  Q, R [rows, H], K, V [source rows, H], Wo [H, H] ([out, in]), bo, gamma, beta [H] (CPU
    tensors of any float type; layouts as in helpers_gpu.attention_ref64).  -> dict of float64 tensors in the launch's row layout:
    ctx, z, y [rows, H], mean, rstd [rows], lse [nseq, nH, Lq]; rows and lse positions that no sequence owns are zero.

    Dropout.  Attention probabilities: helpers_gpu.attention_keep_mask -- row counter (seq * nH + h) * Lq + q with the DENSE Lq, also
    under packing, column = key (xattn.hip `drop_rowkey(seed_a, ((uint64_t)seq * p.nH + h) * p.Lq + qpos)`).  Hidden: row counter
    row_base + (row in the launch's Q tensor), column = channel, ncols = H (`drop_rowkey(seed_h, (uint64_t)(p.row_base + qrow + row))`,
    the counter of spmm_ln_fwd on the whole token batch).

    storage_model=True rounds to bf16 wherever xattn.hip stores or feeds bf16, everything else staying float64:
      * the attention core as attention_ref64(storage_model=True): unnormalised exp * keep rounded (`pack8(st[t], ..)`), the context
        normalised and scaled afterwards and rounded (`ds_wr8(.., to_bf16x4(ot[dt][..] * osc, ..))`: the LDS context panel is bf16,
        and it is that panel which feeds the projection MFMAs and leaves as CTX);
      * x = ctx Wo^T + bo rounded before dropout and residual (epilogue phase 1: `to_bf16x4(acc[a][ct][gq * 4], ..)` into the LDS
        image, "rounded to bf16 exactly as the projection GEMM of the composite rounds it");
      * z = x * keep / (1 - p) + R stays unrounded for the statistics and for y (`sm2 += z[k][m]`, `z[k][m] -= mean2`); Z is its
        rounding as stored (`zb[k][m] = pk2(z[k][m].x, z[k][m].y)`, "rounded before it is centred");
      * y rounded (`o[m] = pk2(y2.x, y2.y)`).
    mean, rstd and lse are fp32 outputs: unrounded.

    defect (one of DEFECTS) is for the tests of the tests only: the output of a kernel with that one defect."""
    assert defect is None or defect in DEFECTS, defect
    H, M = nH * 64, Q.shape[0]
    pa, ph = float(attn_dropout_p), float(hidden_dropout_p)
    lay = dict(nseq=nseq, nH=nH, Lq=Lq, Lkv=Lkv, kmask=kmask, kv_seq=kv_seq, q_row0=q_row0, q_len=q_len, kv_row0=kv_row0, kv_len=kv_len)
    rows = seq_rows(lay)
    rb = _bf16 if storage_model else (lambda t: t)
    keep_a = None
    if pa > 0:
        keep_a = attention_keep_mask(seed, salt_a, nseq, nH, Lq, Lkv, pa, counter_Lq=[n for _, n in rows] if defect == "counter_q_len" else None)
    if defect == "last_key_tile":                    # keys of the last 32-key tile never reach the scores
        km = torch.ones(nseq, Lkv, dtype=torch.int32) if kmask is None else kmask.clone()
        km[:, 32 * (instantiation(H, Lkv)[0] - 1):] = 0
        lay["kmask"] = km
    if defect == "kv_len_unmasked":                  # every source read up to the dense Lkv (as far as the tensor has rows)
        lay["kv_len"] = [min(Lkv, K.shape[0] - r0) for r0 in _ints(kv_row0)]
    O, lse, *_ = attention_ref64(Q, K, V, torch.zeros_like(Q), is_cross=True, p=pa, keep=keep_a, storage_model=storage_model, **lay)
    ctx = torch.zeros(M, H, dtype=torch.float64)
    own = torch.zeros(M, dtype=torch.bool)
    for s, (r0, n) in enumerate(rows):
        ctx[r0:r0 + n] = O[s, :, :n].permute(1, 0, 2).reshape(n, H)
        own[r0:r0 + n] = True
        lse[s, :, n:] = 0
    x = ctx @ Wo.double().t() + bo.double()
    if defect != "x_unrounded_stats_from_Z":
        x = rb(x)
    if ph > 0:
        cnt = [int(row_base) + r for r in range(M)]
        if defect == "row_plus_one":
            cnt = [v + 1 for v in cnt]
        if defect == "row_base_low_word":
            cnt = [(int(row_base) & 0xffffffff) + r for r in range(M)]
        keep_h = torch.from_numpy(_host_dropout_keep(seed, salt_h, np.array(cnt, dtype=np.uint64), H, ph)).double()
        z = (x + R.double()) * keep_h / (1.0 - ph) if defect == "residual_before_mask" else x * keep_h / (1.0 - ph) + R.double()
    else:
        z = x + R.double()
    zs = rb(z) if defect == "x_unrounded_stats_from_Z" else z
    mean = zs.mean(-1)
    var = ((zs - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = rb((z - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double())
    if defect == "neighbour_stats":
        mean, rstd = torch.roll(mean, 1), torch.roll(rstd, 1)
    z = rb(z)
    zero = ~own
    for t in (ctx, z, y, mean, rstd):
        t[zero] = 0
    return dict(ctx=ctx, lse=lse, z=z, mean=mean, rstd=rstd, y=y)


def xattn_lse32(Q, K, V, *, nseq, nH, Lq, Lkv, kmask=None, kv_seq=None, q_row0=None, q_len=None, kv_row0=None, kv_len=None, **_):
    """lse [nseq, nH, Lq] of the same formula with every operation in float32 (the E32 of helpers_gpu.check_ref)."""
    kv_seq, kv_row0, kv_len = _ints(kv_seq), _ints(kv_row0), _ints(kv_len)
    rows = seq_rows(dict(nseq=nseq, Lq=Lq, q_row0=q_row0, q_len=q_len))
    lse = torch.zeros(nseq, nH, Lq, dtype=torch.float32)
    Qf, Kf = Q.float(), K.float()
    for s, (r0, n) in enumerate(rows):
        u = s if kv_seq is None else kv_seq[s]
        k0, nk = (u * Lkv if kv_row0 is None else kv_row0[u]), (Lkv if kv_len is None else kv_len[u])
        q = Qf[r0:r0 + n].view(n, nH, 64).transpose(0, 1)
        k = Kf[k0:k0 + nk].view(nk, nH, 64).transpose(0, 1)
        sc = q @ k.transpose(1, 2) / 8.0
        if kmask is not None:
            sc = sc + (1.0 - kmask[s, :nk].float())[None, None, :] * torch.finfo(torch.float32).min
        lse[s, :, :n] = torch.logsumexp(sc, -1)
    return lse


# ---------------------------------------------------------------------------------------------------------------------
# checker
# ---------------------------------------------------------------------------------------------------------------------
def seq_blocks(t, c, heads=1):
    """Row-layout tensor [rows] or [rows, W] -> float64 [nseq, heads, Lq, W / heads], zero at positions a sequence does not have."""
    t = t.detach().cpu().double()
    t = t[:, None] if t.dim() == 1 else t
    W = t.shape[1] // heads
    out = torch.zeros(c["nseq"], heads, c["Lq"], W, dtype=torch.float64)
    for s, (r0, n) in enumerate(seq_rows(c)):
        out[s, :, :n] = t[r0:r0 + n].reshape(n, heads, W).permute(1, 0, 2)
    return out


def lse_valid(t, c):
    """[nseq, nH, Lq] -> the positions below each sequence's length, as one vector."""
    return torch.cat([t[s, :, :n].reshape(-1) for s, (_, n) in enumerate(seq_rows(c))]).detach().cpu()


def check_xattn(name, got, ref, model, c, lse32):
    """Assert the rules at the head of this module on the six outputs of one launch (`got`: tensors in the launch's layout, any device or
    dtype; rows and lse positions that no sequence owns are not read).  Prints one `[tol]` line per output and a `[tol-row]` line with the
    output of least margin; -> {output: ||got - ref64|| / bound, worst block} ."""
    margin = {}
    for k in ("ctx", "z", "y", "mean", "rstd"):
        heads = c["nH"] if k == "ctx" else 1
        g, r, m = (seq_blocks(t[k], c, heads) for t in (got, ref, model))
        eg, em, bound = attention_parity_blocks(g, r, m)
        margin[k] = (float((eg / bound.clamp_min(1e-300)).max()), _worst_ratio(eg, em))
        check_attention_parity(f"{name} {k}", g, r, m)
    g, r, r32 = (lse_valid(t, c).double() for t in (got["lse"], ref["lse"], lse32))
    margin["lse"] = (float((g - r).abs().max()) / f32_bound(r, r32.float())[1], float("nan"))
    check_ref(f"{name} lse", g, r, r32.float())
    k = max(margin, key=lambda n: margin[n][0])
    print(f"[tol-row] | {name} | {k} | {margin[k][0]:.3f} | {margin[k][1]:.3f} |")
    return {n: v[0] for n, v in margin.items()}


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _case(name, *, H, Lq, Lkv, nseq, kv_seq, holes=False, q_len=None, kv_len=None, pa=0.0, ph=0.0, seed=SEED, salt_a=11, salt_h=22,
          row_base=1000, eps=1e-12, special=None):
    nsrc = max(kv_seq) + 1
    c = dict(name=name, H=H, nH=H // 64, Lq=Lq, Lkv=Lkv, nseq=nseq, nsrc=nsrc, kv_seq=list(kv_seq), kmask=None, q_row0=None, q_len=None,
             kv_row0=None, kv_len=None, pa=pa, ph=ph, seed=seed, salt_a=salt_a, salt_h=salt_h, row_base=row_base, eps=eps, special=special)
    if holes:                                       # a holed key mask per query sequence; key 0 stays visible
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0xffff)
        c["kmask"] = (torch.rand(nseq, Lkv, generator=g) > 0.25).int()
        c["kmask"][:, 0] = 1
    if q_len is not None:
        assert len(q_len) == nseq and max(q_len) == Lq
        c["q_len"] = list(q_len)
        c["q_row0"] = [sum(q_len[:s]) + GAP * s for s in range(nseq)]
        c["q_rows"] = c["q_row0"][-1] + q_len[-1] + GAP
    else:
        c["q_rows"] = nseq * Lq
    if kv_len is not None:
        assert len(kv_len) == nsrc and max(kv_len) == Lkv
        c["kv_len"] = list(kv_len)
        c["kv_row0"] = [sum(kv_len[:u]) for u in range(nsrc)]
        c["kv_rows"] = sum(kv_len)
    else:
        c["kv_rows"] = nsrc * Lkv
    return c


def _tables():
    cases = {}

    def add(table, name, **kw):
        cases[name] = _case(name, **kw)
        table.append(name)

    inst, pan, cnt, ln = [], [], [], []
    # Every instantiation: Lq = 70 (a second panel with 6 valid rows), three sequences on two shared sources
    for nct, H in ((1, 128), (2, 256), (6, 768)):
        for nt in (1, 2, 3, 4):
            base = dict(H=H, Lq=70, nseq=3, kv_seq=[1, 0, 1])
            add(inst, f"nt{nt}-nct{nct}-dense", Lkv=32 * nt, holes=True, **base)                      # upper edge of the tile count
            lo = 31 if nt == 1 else 32 * (nt - 1) + 1                                                 # lower edge (NT = 1: 31, so that > 1 key is in play)
            add(inst, f"nt{nt}-nct{nct}-packed", Lkv=lo, q_len=[70, 33, 65], kv_len=[1, lo], **base)
            add(inst, f"nt{nt}-nct{nct}-drop", Lkv=32 * nt, holes=True, pa=0.1, ph=0.1, **base)
    # Panels: grid.x = 1 .. 5, the edges of the 32-row tile and of the 64-row panel
    for H in (768, 128):
        for Lq in (1, 32, 33, 63, 64, 65, 128, 129, 192, 256, 257, 300):                              # (256: the four-panel launch)
            add(pan, f"panels-h{H}-lq{Lq}", H=H, Lq=Lq, Lkv=54, nseq=2, kv_seq=[1, 0], holes=True)
        add(pan, f"panels-h{H}-packed", H=H, Lq=300, Lkv=54, nseq=4, kv_seq=[1, 0, 0, 1], q_len=[300, 1, 64, 65], holes=True, pa=0.1, ph=0.1)
    # Counters: packed (the dense Lq in the attention counter), row_base beyond 32 bits, high words of seed and salts, a second threshold
    cb = dict(H=128, Lq=70, Lkv=54, nseq=3, kv_seq=[1, 0, 1], q_len=[70, 33, 65], kv_len=[40, 54], holes=True, pa=0.1, ph=0.1)
    add(cnt, "counter-base0", **dict(cb, row_base=0))
    add(cnt, "counter-base1000", **dict(cb, row_base=1000))
    add(cnt, "counter-base2p33", **dict(cb, row_base=2 ** 33 + 1000))
    add(cnt, "counter-highwords", **dict(cb, seed=2 ** 40 + 12345, salt_a=2 ** 33 + 7, salt_h=2 ** 35 + 9))
    add(cnt, "counter-p05", **dict(cb, pa=0.5, ph=0.5))
    # LayerNorm edges
    lb = dict(Lq=70, Lkv=54, nseq=2, kv_seq=[1, 0], holes=True)
    add(ln, "ln-eps1e-5", H=768, eps=1e-5, **lb)
    add(ln, "ln-outlier", H=768, special="outlier", **lb)
    add(ln, "ln-constant-h768", H=768, special="constant", **lb)
    add(ln, "ln-constant-h128", H=128, special="constant", **lb)
    add(ln, "ln-rounding-bias", H=768, special="rounding_bias", **lb)
    return cases, inst, pan, cnt, ln


CASES, INSTANTIATION_CASES, PANEL_CASES, COUNTER_CASES, LN_CASES = _tables()
ALL_CASES = INSTANTIATION_CASES + PANEL_CASES + COUNTER_CASES + LN_CASES


def layout_kw(c):
    """The layout arguments of xattn_ref64 / ops.xattn_fwd out of a case (lists / CPU tensors)."""
    return {k: c[k] for k in ("nseq", "nH", "Lq", "Lkv", "kmask", "kv_seq", "q_row0", "q_len", "kv_row0", "kv_len")}


def ref_kw(c):
    return dict(layout_kw(c), eps=c["eps"], attn_dropout_p=c["pa"], hidden_dropout_p=c["ph"], seed=c["seed"], salt_a=c["salt_a"],
                salt_h=c["salt_h"], row_base=c["row_base"])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(Q, K, V, Wo, bo, R, gamma, beta) of a case: float32 CPU tensors, the first four and R holding bf16 values.  Rows that no sequence
    owns hold values too."""
    c = CASES[name]
    H = c["H"]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(BF).float()
    Q, K, V, R, Wo = r(c["q_rows"], H, scale=1.5), r(c["kv_rows"], H), r(c["kv_rows"], H), r(c["q_rows"], H), r(H, H, scale=0.04)
    bo = 0.1 * torch.randn(H, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    if c["special"] == "outlier":                   # one channel 50 times the others, as the outlier channels of a trained model
        R[:, 77] = (R[:, 77] * 50).to(BF).float()
    elif c["special"] == "constant":                # z = 1.5 in every channel, exactly, in every precision: y = beta
        Wo, bo, R = torch.zeros(H, H), torch.full((H,), 1.0), torch.full((c["q_rows"], H), 0.5)
    elif c["special"] == "rounding_bias":
        # z = (1 + k / 128) + (2^-8 - 2^-16), k in 0 .. 31: x and R are bf16 values, every z rounds DOWN by almost half a bf16 ulp, so
        # the mean of the rounded Z lies 2^-8 / 1.12 = 1.8 x 2^-9 (relative) below the mean of z
        Wo = torch.zeros(H, H)
        bo = 1.0 + torch.randint(0, 32, (H,), generator=g).float() / 128
        R = torch.full((c["q_rows"], H), 2.0 ** -8 - 2.0 ** -16)
    assert all(torch.equal(t, t.to(BF).float()) for t in (Q, K, V, R, Wo))
    return Q, K, V, Wo, bo, R, gamma, beta


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, inputs, float64 reference, storage model, fp32 lse) of a case: computed once, shared, left unchanged."""
    c, x = CASES[name], inputs(name)
    return c, x, xattn_ref64(*x, **ref_kw(c)), xattn_ref64(*x, **ref_kw(c), storage_model=True), xattn_lse32(*x[:3], **layout_kw(c))
