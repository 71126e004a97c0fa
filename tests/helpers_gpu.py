"""Helpers shared by the GPU test modules."""
import math

import numpy as np


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _tiny_train_model(env, dropout=True):
    O, SPMM, tiny_config, *_ = env
    cfg = tiny_config()
    if not dropout:
        for c in (cfg.text, cfg.prop):
            c.hidden_dropout_prob = c.attention_probs_dropout_prob = 0.0
    sched = {'sched': 'cosine', 'lr': 1e-3, 'epochs': 4, 'min_lr': 1e-5, 'decay_rate': 1, 'warmup_lr': 1e-4,
             'warmup_epochs': 2, 'cooldown_epochs': 0}
    tc = {'embed_dim': 64, 'temp': 0.07, 'queue_size': 16, 'momentum': 0.995, 'alpha': 0.4, 'schedular': sched,
          'optimizer': {'opt': 'adamW', 'lr': 1e-3, 'weight_decay': 0.02}}
    m = SPMM(config=tc, spmm_config=cfg, loader_len=10)
    m.load_state_dict(O.closed_form_state_dict(O.tiny_cfg()))
    return m.train()


def _strided(x, extra, lead):
    """x [r, E] on the device inside a wider NaN-filled matrix: row stride E + extra, first element `lead` floats in (16-byte aligned)."""
    import torch
    r, E = x.shape
    w = torch.full((max(r, 1), E + extra), float("nan"), device="cuda")
    v = w[:r, lead:lead + E]
    v.copy_(torch.as_tensor(x))
    return v


# ---------------------------------------------------------------------------------------------------------------------
# Host model of csrc/common.h's counter-based generator: the ONE model of it in the tests.
# ---------------------------------------------------------------------------------------------------------------------
_M64, _M32 = (1 << 64) - 1, np.uint64(0xffffffff)


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _host_seed_mix(seed, salt):
    """seed_mix: two splitmix64 rounds over the per-step seed and the per-call-site salt."""
    return _splitmix64((_splitmix64(seed & _M64) + salt) & _M64)


def _mix32(x):                                      # "lowbias32" on uint64 arrays holding 32-bit values
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x21f0aaad)) & _M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x735a2d97)) & _M32
    return x ^ (x >> np.uint64(15))


def _host_dropout_keep(seed, salt, rows, ncols, p):
    """Host model of csrc/common.h's dropout counter hash: keep[row, col] for `rows` (uint64 row counters) x ncols elements.
    seed_mix (two splitmix64 rounds over seed and salt) -> drop_rowkey (lowbias32 of the row) -> drop_pair (Weyl step + two 24-bit
    multiply rounds) -> one 16-bit half per element against round(p * 65536).  The statistics of THIS function were checked against
    lowbias32 when it was adopted (EXPERIMENTS.md 1.7); test_kernels_gpu.py::test_dropout_masks_equal_the_host_model_of_the_hash pins
    the kernels to it bit for bit."""
    def mix24(x):
        x = x ^ (x >> np.uint64(16)); x = ((x & np.uint64(0xffffff)) * np.uint64(0xda8f81)) & _M32
        x = x ^ (x >> np.uint64(16)); x = ((x & np.uint64(0xffffff)) * np.uint64(0x76dfb5)) & _M32
        return x ^ (x >> np.uint64(16))

    s64 = _host_seed_mix(seed, salt)
    s_lo, s_hi = np.uint64(s64 & 0xffffffff), np.uint64(s64 >> 32)
    rows = np.asarray(rows, dtype=np.uint64)
    rowkey = _mix32((rows & _M32) ^ s_lo) ^ s_hi ^ (((rows >> np.uint64(32)) * np.uint64(0x9E3779B1)) & _M32)
    pair = np.arange(ncols // 2, dtype=np.uint64)
    r = mix24((rowkey[:, None] + pair[None, :] * np.uint64(0x9E3779B1)) & _M32)
    u = np.stack([r & np.uint64(0xffff), r >> np.uint64(16)], axis=2).reshape(len(rows), ncols)
    return u >= np.uint64(int(p * 65536 + 0.5))


def _host_rng_uniform(seed, salt, idx):
    """Host model of rng_uniform(seed_mix(seed, salt), idx) = (rng_pair(...) >> 8) / 2^24, exact in float64, for an array of indices.
    rng_pair = lowbias32((idx_lo ^ seed_lo) + (idx_hi ^ seed_hi) * 0x9E3779B1)."""
    s64 = _host_seed_mix(seed, salt)
    s_lo, s_hi = np.uint64(s64 & 0xffffffff), np.uint64(s64 >> 32)
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = idx & _M32, idx >> np.uint64(32)
    r = _mix32(((lo ^ s_lo) + (((hi ^ s_hi) * np.uint64(0x9E3779B1)) & _M32)) & _M32)
    return (r >> np.uint64(8)).astype(np.float64) / 16777216.0


# ---------------------------------------------------------------------------------------------------------------------
# Tolerances of the per-kernel tests that compare with a float64 reference (test_loss_kernels_gpu.py,
# test_optim_and_small_kernels_gpu.py).  The bound is derived from the reference alone:
#   E32   = largest error of the SAME formula evaluated in fp32 torch on the CPU against its float64 evaluation
#   bound = max(8 * E32, 4 fp32 ulp of the output's largest magnitude)        (8: __expf against expf, another summation order)
#   a bf16 output may additionally be one bf16 ulp of the reference (relative 2^-7) away, element by element.
# ---------------------------------------------------------------------------------------------------------------------
def f32_bound(ref64, ref32):
    E32 = (ref32.double() - ref64).abs().max().item()
    mag = ref64.abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(mag)) - 23) if mag > 0 else 0.0
    return E32, max(8 * E32, 4 * ulp)


def check_ref(name, got, ref64, ref32, bf16=False):
    """Assert |got - ref64| <= bound (see above) element by element; prints E32, the kernel's error and the bound."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    ref32 = ref32.detach().reshape(ref64.shape)
    E32, bound = f32_bound(ref64, ref32)
    err = (got - ref64).abs()
    allow = bound + (2.0 ** -7) * ref64.abs() if bf16 else bound + 0 * ref64
    over = (err - ((2.0 ** -7) * ref64.abs() if bf16 else 0)).max().item()      # what the fp32 part of the bound has to cover
    print(f"[tol] {name}: E32={E32:.3e} kernel={err.max().item():.3e}{f' (past 1 bf16 ulp: {max(over, 0):.3e})' if bf16 else ''} "
          f"bound={bound:.3e}{' + 2^-7|ref|' if bf16 else ''}")
    ok = err <= allow                                                         # (NaN compares false)
    assert ok.all(), f"{name}: {int((~ok).sum())}/{ok.numel()} off; max err {err.max().item():.4g} (E32 {E32:.3g}, bound {bound:.3g}, " \
                     f"ref max {ref64.abs().max().item():.4g}) first bad idx {(~ok).nonzero()[0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# Attention with dropout: float64 reference, bf16 storage model, mask probes (tests/test_attention_dropout_gpu.py; the
# helpers test themselves on the CPU in tests/test_attention_reference_cpu.py).
#
# Launches are described as csrc/attention.hip takes them: token-major [rows, nH * 64] tensors, dense rows (row = seq * L + pos) or
# packed rows (q_row0 / q_len per query sequence, kv_row0 / kv_len per key/value source), kv_seq[s] = source read by query sequence s
# (dK / dV then per QUERY sequence, dense), kmask [nseq, Lkv] per query sequence.  Results come back in ONE canonical dense form,
# [sequence, head, position, 64] float64 with zeros at positions a sequence does not have: attn_heads() brings a kernel's output there.
# ---------------------------------------------------------------------------------------------------------------------
def _ints(x):
    return None if x is None else [int(v) for v in (x.tolist() if hasattr(x, "tolist") else x)]


def attn_heads(t, n, L, nH, row0=None, lens=None):
    """Token-major [rows, >= nH * 64] tensor (any device / dtype) -> float64 CPU [n, nH, L, 64]; sequence s owns lens[s] rows from
    row0[s] (None: dense, L rows from s * L); positions past lens[s] are zero."""
    import torch
    t = t.detach().cpu().double()
    row0, lens = _ints(row0), _ints(lens)
    out = torch.zeros(n, nH, L, 64, dtype=torch.float64)
    for s in range(n):
        r0, ln = (s * L if row0 is None else row0[s]), (L if lens is None else lens[s])
        out[s, :, :ln] = t[r0:r0 + ln, :nH * 64].reshape(ln, nH, 64).permute(1, 0, 2)
    return out


def attn_visible(*, nseq, Lq, Lkv, kmask=None, causal_from=None, is_cross=False, kv_seq=None, q_len=None, kv_len=None, **_):
    """bool [nseq, Lq, Lkv]: the (query, key) pairs with a non-zero probability -- inside q_len / kv_len, kmask = 1, not above the diagonal
    of a causal sequence.  (Every row of the test cases keeps at least one such key, so every other key's probability is exactly 0.)"""
    import torch
    kv_seq, q_len, kv_len = _ints(kv_seq), _ints(q_len), _ints(kv_len)
    cf = nseq if (causal_from is None or is_cross) else causal_from
    qi, ki = torch.arange(Lq)[:, None], torch.arange(Lkv)[None, :]
    vis = torch.zeros(nseq, Lq, Lkv, dtype=torch.bool)
    for s in range(nseq):
        u = s if kv_seq is None else kv_seq[s]
        v = (qi < (Lq if q_len is None else q_len[s])) & (ki < (Lkv if kv_len is None else kv_len[u]))
        if kmask is not None:
            v = v & (kmask[s].cpu()[None, :] != 0)
        if s >= cf:
            v = v & (ki <= qi)
        vis[s] = v
    return vis


def attention_keep_mask(seed, salt, nseq, nH, Lq, Lkv, p, counter_Lq=None):
    """bool [nseq, nH, Lq, Lkv] keep mask of one attention launch from the host model of the hash: element (seq, h, q, kv) uses the row
    counter (seq * nH + h) * Lq + q with the launch's DENSE Lq (also in packed layouts) and column kv.  counter_Lq (an int or one per
    sequence) replaces that Lq: only the tests of the tests use it, to build a wrong mask."""
    import torch
    cl = [Lq] * nseq if counter_Lq is None else ([int(counter_Lq)] * nseq if np.ndim(counter_Lq) == 0 else _ints(counter_Lq))
    rows = np.array([[[(s * nH + h) * cl[s] + q for q in range(Lq)] for h in range(nH)] for s in range(nseq)], dtype=np.uint64)
    ncols = Lkv + (Lkv & 1)
    keep = _host_dropout_keep(seed, salt, rows.reshape(-1), ncols, p)[:, :Lkv]
    return torch.from_numpy(np.ascontiguousarray(keep)).reshape(nseq, nH, Lq, Lkv)


def _bf16(x):
    import torch
    return x.float().to(torch.bfloat16).double()


def attention_ref64(Q, K, V, dO, *, nseq, nH, Lq, Lkv, kmask=None, causal_from=None, is_cross=False, p=0.0, keep=None, seed=None, salt=0,
                    kv_seq=None, q_row0=None, q_len=None, kv_row0=None, kv_len=None, storage_model=False, dp_scale=None):
    """Float64 attention forward and backward of one launch, written out (no autograd):

        s  = Q K^T / 8 + additive mask        self: -10000 at kmask = 0 and, for sequences >= causal_from, above the diagonal (once);
                                              cross: finfo(float32).min at kmask = 0  (the arithmetic of test_kernels_gpu.py::ref_attention)
        P  = softmax(s),  lse = logsumexp(s)
        P~ = P * keep / (1 - p),              O  = P~ V
        dP = (dO V^T) * keep / (1 - p),       D  = sum_kv P dP,      dS = P (dP - D)
        dQ = dS K / 8,    dK = dS^T Q / 8,    dV = P~^T dO

    keep [nseq, nH, Lq, Lkv] is given, or drawn by attention_keep_mask(seed, salt, ...) (the host model of the generator); p = 0: all ones.
    Inputs in the launch's layout (see the head of this section); -> O, lse, dQ, dK, dV with O, dQ [nseq, nH, Lq, 64], lse [nseq, nH, Lq],
    dK, dV [nseq, nH, Lkv, 64] -- per QUERY sequence, which is the key/value source itself unless kv_seq is given (the ABI's rule).

    storage_model=True evaluates the same formulas with a bf16 rounding wherever csrc/attention.hip stores or feeds bf16 (its comments at
    the PV product, at `ppk` / `dpk` and at the stores), everything else staying float64:
      * forward: the UNNORMALISED probabilities exp(s - max) * keep are rounded, multiplied into V, and the sum is normalised (1 / sum of
        the unrounded, undropped exp) and scaled by 1 / (1 - p) afterwards;
      * backward: P is rounded (`ppk`) -- after D = sum P dP was taken from the unrounded P;
      * dS = bf16(bf16(P) * (dP - D)) (`dpk`), with dP only MASKED: the kernels apply 1 / (1 - p) once, to the dQ / dK / dV accumulators;
      * P~ = bf16(P) * keep (the same rounded P, masked; scaled at the dV store);
      * the outputs O, dQ, dK, dV.
    D and lse stay unrounded.  (Not modelled: the launch per 128-query chunk adds its dK / dV to the bf16 result of the chunk before --
    one more rounding; the chunked path beyond 256 tokens rounds every chunk pair's O, dQ, dK, dV before they are summed in fp32.)

    dp_scale replaces the 1 / (1 - p) of dP (hence of dQ and dK): only the tests of the tests use it."""
    import torch
    kv_seq, q_len, kv_len = _ints(kv_seq), _ints(q_len), _ints(kv_len)
    nsrc = len(kv_row0) if kv_row0 is not None else K.shape[0] // Lkv
    Qd, dOd = attn_heads(Q, nseq, Lq, nH, q_row0, q_len), attn_heads(dO, nseq, Lq, nH, q_row0, q_len)
    Kd, Vd = attn_heads(K, nsrc, Lkv, nH, kv_row0, kv_len), attn_heads(V, nsrc, Lkv, nH, kv_row0, kv_len)
    if keep is None:
        keep = attention_keep_mask(seed, salt, nseq, nH, Lq, Lkv, p) if p > 0 else torch.ones(nseq, nH, Lq, Lkv, dtype=torch.bool)
    cf = nseq if (causal_from is None or is_cross) else causal_from
    sc_p = 1.0 / (1.0 - p)
    sc_dp = sc_p if dp_scale is None else dp_scale
    rb = _bf16 if storage_model else (lambda x: x)
    O, dQ = torch.zeros(nseq, nH, Lq, 64, dtype=torch.float64), torch.zeros(nseq, nH, Lq, 64, dtype=torch.float64)
    dK, dV = torch.zeros(nseq, nH, Lkv, 64, dtype=torch.float64), torch.zeros(nseq, nH, Lkv, 64, dtype=torch.float64)
    lse = torch.zeros(nseq, nH, Lq, dtype=torch.float64)
    for s in range(nseq):
        u = s if kv_seq is None else kv_seq[s]
        nq, nk = (Lq if q_len is None else q_len[s]), (Lkv if kv_len is None else kv_len[u])
        q, do, k, v = Qd[s, :, :nq], dOd[s, :, :nq], Kd[u, :, :nk], Vd[u, :, :nk]
        m = torch.ones(nk, dtype=torch.float64) if kmask is None else kmask[s, :nk].cpu().double()
        if is_cross:
            add = ((1 - m) * torch.finfo(torch.float32).min)[None, :].expand(nq, nk)
        else:
            ext = m[None, :].expand(nq, nk)
            if s >= cf:
                ext = ext * (torch.arange(nk)[None, :] <= torch.arange(nq)[:, None]).double()
            add = (1 - ext) * -10000.0
        sc = q @ k.transpose(-1, -2) / 8.0 + add
        l = torch.logsumexp(sc, dim=-1)
        kp = keep[s, :, :nq, :nk].double()
        P = torch.exp(sc - l[..., None])
        dPm = (do @ v.transpose(-1, -2)) * kp                          # masked, unscaled
        D = (P * dPm).sum(-1, keepdim=True)
        if storage_model:
            e = torch.exp(sc - sc.max(-1, keepdim=True).values)
            o = rb((rb(e * kp) @ v) / e.sum(-1, keepdim=True) * sc_p)
        else:
            o = (P * kp) @ v * sc_p
        Pb = rb(P)
        dS = rb(Pb * (dPm - D))
        Pt = Pb * kp
        O[s, :, :nq], lse[s, :, :nq] = o, l
        dQ[s, :, :nq] = rb((dS @ k) * (0.125 * sc_dp))
        dK[s, :, :nk] = rb((dS.transpose(-1, -2) @ q) * (0.125 * sc_dp))
        dV[s, :, :nk] = rb((Pt.transpose(-1, -2) @ do) * sc_p)
    return O, lse, dQ, dK, dV


def _worst_ratio(eg, em):
    nz = em > 0
    return float((eg[nz] / em[nz]).max()) if bool(nz.any()) else 0.0


def attention_parity_blocks(got, ref64, model):
    """-> per block [n, nH]: ||got - ref64||, ||model - ref64||, the bound 2 ||model - ref64|| + 2^-9 ||ref64||."""
    eg = (got - ref64).flatten(2).norm(dim=-1)
    em = (model - ref64).flatten(2).norm(dim=-1)
    return eg, em, 2 * em + 2.0 ** -9 * ref64.flatten(2).norm(dim=-1)


def check_attention_parity(name, got, ref64, model):
    """Per (sequence, head) block of [n, nH, L, 64] tensors: ||got - ref64|| <= 2 ||model - ref64|| + 2^-9 ||ref64||.  The storage model holds
    every bf16 rounding the kernels document; the factor 2 is for what it does not hold (fp32 summation order, __expf, the second query
    chunk's bf16 add of dK / dV: +18-26 % measured); 2^-9 ||ref64|| is half a bf16 ulp of the output, for blocks where the model's error
    happens to be zero.  Prints the worst ratio ||got - ref64|| / ||model - ref64||; -> that ratio."""
    eg, em, bound = attention_parity_blocks(got, ref64, model)
    ratio = _worst_ratio(eg, em)
    print(f"[tol] {name}: worst ||got - ref64|| / ||model - ref64|| = {ratio:.3f} over {eg.numel()} blocks "
          f"(model error {em.min().item():.2e} .. {em.max().item():.2e}, relative {(em / ref64.flatten(2).norm(dim=-1).clamp_min(1e-300)).max().item():.2e})")
    ok = eg <= bound                                                          # (NaN compares false)
    assert ok.all(), f"{name}: {int((~ok).sum())}/{ok.numel()} blocks over the bound; worst ratio {ratio:.3f}; first bad block " \
                     f"{(~ok).nonzero()[0].tolist()}: error {eg[~ok][0].item():.3e}, bound {bound[~ok][0].item():.3e}"
    return ratio


# ---- mask probes.  Q = 0 in all of them: every visible key of a row has the same positive probability 1 / n whatever K is.
PROBE_C = 4.0                                        # dO[q] . v of the dP probe: dO rows and V rows are all 0.25 * ones(64)


def probe_unit_rows(rows, nH, off, n, L, row0=None, lens=None):
    """[rows, nH * 64] float32: the row of position pos of every sequence is the unit vector e_(pos - off) in every head when
    off <= pos < off + 64, else zero.  As V: O[q][d] = P~[q][off + d]; as K: dQ[q][d] = dS[q][off + d] / 8; as dO: dV[kv][d] = P~[off + d][kv]."""
    import torch
    row0, lens = _ints(row0), _ints(lens)
    M = torch.zeros(rows, 64)
    for s in range(n):
        r0, ln = (s * L if row0 is None else row0[s]), (L if lens is None else lens[s])
        for pos in range(off, min(off + 64, ln)):
            M[r0 + pos, pos - off] = 1.0
    return M.repeat(1, nH)


def probe_keep_from_fwd(O_passes, Lkv):
    """Forward probe: O of the passes off = 0, 64, .. with V = probe_unit_rows -> keep [nseq, nH, Lq, Lkv] (False where invisible)."""
    import torch
    return (torch.cat(O_passes, dim=-1)[..., :Lkv] != 0)


def probe_keep_from_dv(dV_passes, Lq):
    """P~ probe: dV of the passes q0 = 0, 64, .. with dO = probe_unit_rows -> keep [nseq, nH, Lq, Lkv] (False where invisible)."""
    import torch
    return (torch.cat(dV_passes, dim=-1)[..., :Lq] != 0).transpose(-1, -2)


def probe_keep_from_dq(dQ_passes, vis, p):
    """dP probe: dQ of the passes off = 0, 64, .. with K = probe_unit_rows, every V row and every dO row 0.25 * ones(64).  Then
    dP = PROBE_C * keep / (1 - p) for every key of a row, D = PROBE_C f / (1 - p) with f the kept share of the row's n visible keys, and
    dQ[q][kv - off] = delta * (keep - f), delta = PROBE_C / ((1 - p) 8 n): two values per row, delta apart.  Threshold at their midpoint.
    A row whose visible keys were ALL kept or ALL dropped has dS = 0 identically (the softmax gradient of a constant dP): its dP mask
    reaches no output and cannot be read from any; such rows come back in `flat`.
    -> keep [nseq, nH, Lq, Lkv], flat [nseq, nH, Lq] (bool), worst distance of a visible value from its row's two levels in units of delta."""
    import torch
    X = torch.cat(dQ_passes, dim=-1)[..., :vis.shape[-1]]
    v = vis[:, None].expand_as(X)
    n = vis.sum(-1).clamp_min(1)[:, None, :, None].double()
    delta = PROBE_C / ((1.0 - p) * 8.0 * n)
    hi = torch.where(v, X, torch.full_like(X, -float("inf"))).max(-1, keepdim=True).values
    lo = torch.where(v, X, torch.full_like(X, float("inf"))).min(-1, keepdim=True).values
    flat = ((hi - lo) < 0.5 * delta).squeeze(-1) | ~vis.any(-1)[:, None]
    keep = (X > 0.5 * (hi + lo)) & v
    off = torch.minimum((X - hi).abs(), (X - lo).abs()) / delta
    return keep, flat, float(torch.where(v, off, torch.zeros_like(off)).max())


def probe_dq_mismatches(keep_dq, flat, want, vis):
    """Visible decisions on which the dP probe contradicts `want`: on the rows it can read, every differing decision; a flat row
    contradicts `want` when want's visible decisions of that row are not all equal (then all of them count)."""
    v = vis[:, None].expand_as(want)
    diff = ((keep_dq != want) & v & ~flat[..., None]).sum()
    kept = (want & v).sum(-1)
    mixed = (kept > 0) & (kept < v.sum(-1))
    return int(diff) + int((v.sum(-1) * (flat & mixed)).sum())


def probe_fwd_mask(run, c):
    """The forward probe alone (see probe_masks)."""
    import torch
    nH, H, qr, kr = c["nH"], c["nH"] * 64, c["q_rows"], c["kv_rows"]
    g = torch.Generator().manual_seed(6)
    Z, Kr, dOr = torch.zeros(qr, H), torch.randn(kr, H, generator=g), torch.randn(qr, H, generator=g)
    return probe_keep_from_fwd([run(Z, Kr, probe_unit_rows(kr, nH, off, c["nsrc"], c["Lkv"], c["kv_row0"], c["kv_len"]), dOr, False)[0]
                                for off in range(0, c["Lkv"], 64)], c["Lkv"])


def probe_masks(run, c):
    """The three probes of one case.  run(Q, K, V, dO, bwd) -> (O, dQ, dK, dV) in the canonical form (dQ, dK, dV unused when bwd is false)
    runs the launch of case c on float32 CPU inputs in the launch's layout -- the kernels, or attention_ref64 with a known mask.
    -> keep of the forward, keep of the P~ path, (keep, flat rows, level spread) of the dP path."""
    import torch
    nH, H, qr, kr = c["nH"], c["nH"] * 64, c["q_rows"], c["kv_rows"]
    g = torch.Generator().manual_seed(5)
    Z, Kr, Vr, dOr = torch.zeros(qr, H), torch.randn(kr, H, generator=g), torch.randn(kr, H, generator=g), torch.randn(qr, H, generator=g)
    unit_kv = lambda off: probe_unit_rows(kr, nH, off, c["nsrc"], c["Lkv"], c["kv_row0"], c["kv_len"])
    unit_q = lambda off: probe_unit_rows(qr, nH, off, c["nseq"], c["Lq"], c["q_row0"], c["q_len"])
    vis = attn_visible(**attention_layout_kw(c))
    fw = probe_fwd_mask(run, c)
    dv = probe_keep_from_dv([run(Z, Kr, Vr, unit_q(q0), True)[3] for q0 in range(0, c["Lq"], 64)], c["Lq"])
    dq = probe_keep_from_dq([run(Z, unit_kv(off), torch.full((kr, H), 0.25), torch.full((qr, H), 0.25), True)[1]
                             for off in range(0, c["Lkv"], 64)], vis, c["p"])
    return fw, dv, dq


def attention_dropout_case(name):
    """The launches of tests/test_attention_dropout_gpu.py (and, for a and f, of the CPU tests of these helpers): the smallest shapes that
    reach each code path of csrc/attention.hip with dropout on.  -> dict of the launch (lists / CPU tensors; `q_rows`, `kv_rows`: rows of
    the query and key/value tensors)."""
    import torch
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    c = dict(nH=2, p=0.1, seed=20261018, salt=1000 + ord(name[0]), is_cross=False, causal_from=None, kmask=None, kv_seq=None,
             q_row0=None, q_len=None, kv_row0=None, kv_len=None)
    cum0 = lambda ls: [sum(ls[:i]) for i in range(len(ls))]
    if name == "a":          # <= 128-key backward; a non-causal and two causal sequences in one launch; prefix key mask
        c.update(nseq=3, Lq=54, Lkv=54, causal_from=1, kmask=(torch.arange(54)[None, :] < torch.tensor([54, 40, 29])[:, None]).int())
    elif name == "b":        # packed self-attention: dense counter indexing under packing; one- and two-token sequences
        ls = [100, 1, 2, 17, 64]
        c.update(nseq=5, Lq=100, Lkv=100, causal_from=2, q_row0=cum0(ls), q_len=ls, kv_row0=cum0(ls), kv_len=ls)
    elif name == "c":        # the step's cross form: packed on both sides, two shared sources
        ql, kl = [54, 20, 37, 5, 48], [128, 77]
        c.update(nseq=5, Lq=54, Lkv=128, is_cross=True, kv_seq=[0, 1, 1, 0, 1], q_row0=cum0(ql), q_len=ql, kv_row0=cum0(kl), kv_len=kl)
    elif name == "d":        # 54 keys = three 16-key tiles + 6; masked keys inside a tile
        km = (torch.rand(4, 54, generator=g) > 0.25).int()
        km[:, 0] = 1
        c.update(nseq=4, Lq=128, Lkv=54, is_cross=True, kv_seq=[0, 1, 1, 0], kmask=km, nsrc=2)
    elif name == "e":        # 256-key backward (key halves on two waves), two query chunks
        ls = [200, 129, 31]
        c.update(nseq=3, Lq=200, Lkv=200, causal_from=1, q_row0=cum0(ls), q_len=ls, kv_row0=cum0(ls), kv_len=ls)
    elif name in ("f1", "f2"):   # each long side alone
        Lq, Lkv = (54, 256) if name == "f1" else (256, 54)
        c.update(nseq=2, Lq=Lq, Lkv=Lkv, is_cross=True)
    elif name in ("g54", "g200"):   # engine.SelfKV: one query row per sequence over kv_row0 / kv_len in another tensor
        L = int(name[1:])
        kl = [L, 3, L // 2, L - 1, 17, L // 3]
        c.update(nseq=6, Lq=1, Lkv=L, causal_from=6, kv_row0=cum0(kl), kv_len=kl)
    elif name == "h":        # odd key count, odd head count, the high words of seed and salt, a second threshold
        c.update(nseq=2, nH=3, Lq=33, Lkv=77, is_cross=True, p=0.5, seed=2 ** 40 + 12345, salt=2 ** 33 + 7)
    elif name == "i":        # beyond 256 tokens: the chunked path of ops.attn_fwd_long / attn_bwd_long
        c.update(nseq=2, Lq=300, Lkv=300, causal_from=1)
    else:
        raise KeyError(name)
    nsrc = c.pop("nsrc", None)
    if nsrc is None:
        nsrc = len(c["kv_len"]) if c["kv_len"] is not None else c["nseq"]
    c["nsrc"] = nsrc
    c["q_rows"] = sum(c["q_len"]) if c["q_len"] is not None else c["nseq"] * c["Lq"]
    c["kv_rows"] = sum(c["kv_len"]) if c["kv_len"] is not None else nsrc * c["Lkv"]
    return c


def attention_layout_kw(c):
    """The arguments of attention_ref64 / attn_visible out of a case dict."""
    return {k: c[k] for k in ("nseq", "nH", "Lq", "Lkv", "kmask", "causal_from", "is_cross", "kv_seq", "q_row0", "q_len", "kv_row0", "kv_len")}
