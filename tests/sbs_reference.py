"""Float64 NumPy restatement of stochastic beam search (Kool, van Hoof, Welling 2019) as spmm_sbs_step defines it (include/spmm_hip.h):
one step for G groups x W slots, the whole search over a callable model, a toy model with 15 sequences whose probabilities are known, and
the checks the CPU and the GPU tests share.  Not a test module: tests/test_sbs_reference_cpu.py tests it (seeded defects included)."""
import numpy as np

CLS, SEP = 2, 3
ALLOWED_ABOVE = -1e29
MASKED = -1e30
NEG = -np.inf
DEFECTS = ("unconditioned", "lse_all", "ties_high", "finished_many")
# 4 x the largest |kernel key - float64 key| measured over the cases of tests/test_sbs_step_gpu.py on an MI355X (5.578e-6, at G, W, V = 1, 1024, 512):
# what the GPU tests allow between spmm_sbs_step's fp32 keys and this file's.  The margin of 4 is for other boxes and compiler versions.
DELTA = 2.24e-5


def candidates_ref(logits, noise, phi, gum, fin, defect=None, raw=None):
    """logits, noise [G, W, V]; phi, gum [G, W] float64; fin [G, W] bool -> (key, cphi) [G, W, V]: the key (-inf: no candidate) and the
    log-probability of every (slot, token).  defect: one of DEFECTS (a deliberately wrong variant); raw: the logits before the mask."""
    l, nz = np.asarray(logits, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    T, phi, fin = np.asarray(gum, dtype=np.float64), np.asarray(phi, dtype=np.float64), np.asarray(fin).astype(bool)
    used = T > NEG                                                         # (NaN: empty)
    live, done = used & ~fin, used & fin
    ok = (l > ALLOWED_ABOVE) & live[..., None]
    with np.errstate(all="ignore"):
        src = np.where(ok, l, NEG) if defect != "lse_all" else np.where(live[..., None], np.asarray(raw, dtype=np.float64), NEG)
        m = src.max(-1, keepdims=True)
        m0 = np.where(np.isfinite(m), m, 0.0)
        lse = m0 + np.log(np.exp(src - m0).sum(-1, keepdims=True))
        cphi = phi[..., None] + (l - lse)
        g = np.where(ok, cphi + nz, NEG)
        Z = g.max(-1, keepdims=True)
        v = T[..., None] - g + np.log1p(-np.exp(g - Z))
        key = T[..., None] - np.maximum(0.0, v) - np.log1p(np.exp(-np.abs(v)))
        if defect == "unconditioned":
            key = g
    key = np.where(ok & ~np.isnan(key), key, NEG)
    key[..., SEP] = np.where(done, T, key[..., SEP])
    cphi[..., SEP] = np.where(done, phi, cphi[..., SEP])
    if defect == "finished_many":                                         # a finished slot offers itself twice
        key[..., SEP + 1] = np.where(done, T, key[..., SEP + 1])
        cphi[..., SEP + 1] = np.where(done, phi, cphi[..., SEP + 1])
    return key, cphi


def select_ref(key, W, defect=None):
    """key [G, W*V] -> (flat [G, W] the W best by (key descending, flat index ascending), their keys; -inf keys are never selected: have)."""
    if defect == "ties_high":
        n = key.shape[1]
        flat = n - 1 - np.argsort(-key[:, ::-1], axis=1, kind="stable")[:, :W]
    else:
        flat = np.argsort(-key, axis=1, kind="stable")[:, :W]
    skey = np.take_along_axis(key, flat, axis=1)
    return flat, skey, skey > NEG


def new_state_ref(flat, skey, have, cphi, phi, fin, length, tokens, anc, t, V):
    """The state spmm_sbs_step writes for the selection (flat, skey, have) -> dict(phi, gum, fin, len, tokens, anc, ids, parent, open)."""
    G, W = flat.shape
    L = tokens.shape[-1]
    parent = np.where(have, flat // V, np.arange(W)[None, :])
    tok = np.where(have, flat % V, 0)
    fin = np.asarray(fin).astype(bool)
    pfin = np.take_along_axis(fin, parent, axis=1) & have
    nfin = have & (pfin | (tok == SEP))
    out = dict(parent=parent, tok=tok)
    out["gum"] = np.where(have, skey, NEG)
    out["phi"] = np.where(have, np.take_along_axis(cphi.reshape(G, -1), flat, axis=1), NEG)
    out["fin"] = nfin
    out["len"] = np.where(have, np.where(pfin, np.take_along_axis(np.asarray(length), parent, axis=1), t + 1), 0)
    tk = np.take_along_axis(np.asarray(tokens), parent[:, :, None], axis=1).copy()
    tk[:, :, t] = np.where(pfin, tk[:, :, t], tok)
    out["tokens"] = np.where(have[:, :, None], tk, 0)
    rows = np.arange(G * W).reshape(G, W)
    prow = (rows[:, :1] + parent).reshape(-1)
    inherit = (np.arange(L)[None, :] < t) & have.reshape(-1, 1)
    anc = np.asarray(anc).reshape(G * W, -1)[:, :L]
    out["anc"] = np.where(inherit, np.clip(anc[prow], 0, G * W - 1), rows.reshape(-1, 1))
    out["ids"] = np.where(have & ~nfin, tok, 0).reshape(-1)
    out["open"] = (have & ~nfin).sum(1)
    return out


def step_ref(logits, noise, state, t, defect=None, raw=None):
    """One position: state = dict(phi, gum, fin, len, tokens [G, W, L], anc [G*W, >= L]) -> the next state (new_state_ref's dict, plus the
    candidate keys `key` [G, W*V] the selection was made from)."""
    G, W, V = logits.shape
    key, cphi = candidates_ref(logits, noise, state["phi"], state["gum"], state["fin"], defect, raw)
    flat, skey, have = select_ref(key.reshape(G, W * V), W, defect)
    out = new_state_ref(flat, skey, have, cphi, state["phi"], state["fin"], state["len"], state["tokens"], state["anc"], t, V)
    out["key"] = key.reshape(G, W * V)
    return out


def start_state(G, W, L, prefix=(CLS,)):
    P = len(prefix)
    tokens = np.zeros((G, W, L), dtype=np.int64)
    tokens[:, :, :P] = np.asarray(prefix)
    phi, gum = np.full((G, W), NEG), np.full((G, W), NEG)
    phi[:, 0] = gum[:, 0] = 0.0
    return dict(phi=phi, gum=gum, fin=np.zeros((G, W), dtype=bool), len=np.full((G, W), P), tokens=tokens,
                anc=np.arange(G * W)[:, None].repeat(L, axis=1)), P


def search_ref(model, noise, G, W, steps, L, defect=None, raw_model=None):
    """The whole search: model(t, tokens [G, W, L]) -> logits [G, W, V] for the token at position t (t tokens held); noise(t, G, W) ->
    [G, W, V] keyed by the position of the last token held; `steps` positions.  -> the final state."""
    state, t = start_state(G, W, L)
    for _ in range(steps):
        lg = model(t, state["tokens"])
        state = step_ref(lg, noise(t - 1, G, W), state, t, defect, None if raw_model is None else raw_model(t, state["tokens"]))
        t += 1
    return state


def sequences(state, n_first=None):
    """-> per group the finished token tuples among the first n_first slots, in slot order."""
    G, W = state["gum"].shape
    n_first = W if n_first is None else n_first
    return [[tuple(int(x) for x in state["tokens"][g, s, : int(state["len"][g, s])]) for s in range(n_first)
             if state["gum"][g, s] > NEG and state["fin"][g, s]] for g in range(G)]


# ---------------------------------------------------------------------------------------------------------------------
# The toy model: V = 6, tokens 0-2 never generated, [SEP] = 3 forced after three free choices -> 1 + 2 + 4 + 8 = 15 sequences
# ---------------------------------------------------------------------------------------------------------------------
TOY_V, TOY_L, TOY_STEPS = 6, 8, 4
TAB = np.random.RandomState(0).randn(4, 6, 6) * 1.5


def toy_raw(t, tokens):
    """Unmasked logits: TAB[position, last token]; t = tokens held (position 0 is [CLS])."""
    return TAB[min(t - 1, 3)][np.asarray(tokens)[..., t - 1] % TOY_V]


def toy_model(t, tokens):
    lg = toy_raw(t, tokens).copy()
    lg[..., :SEP] = MASKED
    if t - 1 >= 3:
        lg[..., SEP + 1:] = MASKED
    return lg


def toy_sequences():
    """{token tuple ([CLS] .. [SEP]): probability} of the 15 sequences."""
    out = {}

    def walk(seq, logp):
        t = len(seq)
        lg = toy_model(t, np.asarray(seq + [0] * (TOY_L - t)))
        okk = lg > ALLOWED_ABOVE
        lp = lg - np.log(np.exp(lg[okk]).sum())
        for v in np.nonzero(okk)[0]:
            if v == SEP:
                out[tuple(seq + [SEP])] = float(np.exp(logp + lp[v]))
            else:
                walk(seq + [int(v)], logp + lp[v])
    walk([CLS], 0.0)
    return out


def toy_noise(seed):
    """The project's counter noise (decode.gumbel_noise_host, k = 8, molecule g * 128 + slot // 8): keyed independently of W."""
    from spmm_amd import decode

    def noise(t, G, W):
        R = (W + 7) // 8
        mols = (np.arange(G)[:, None] * 128 + np.arange(R)[None, :]).reshape(-1)
        z = decode.gumbel_noise_host(seed, decode.DISTINCT_SALT, mols.tolist(), t, 8, TOY_V, TOY_L).numpy()
        return z.reshape(G, R * 8, TOY_V)[:, :W]
    return noise


def inclusion_w2(p):
    """Probability that sequence i is among the two drawn without replacement: p_i + sum_{j != i} p_j p_i / (1 - p_j)."""
    p = np.asarray(p, dtype=np.float64)
    return p + np.array([sum(p[j] * p[i] / (1 - p[j]) for j in range(len(p)) if j != i) for i in range(len(p))])


def sigma_deviation(count, n, p):
    """Largest |observed frequency - p| in units of sigma = sqrt(p (1 - p) / n)."""
    count, p = np.asarray(count, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return float(np.max(np.abs(count / n - p) / np.sqrt(p * (1 - p) / n)))


def toy_statistics(firsts, pairs):
    """firsts: the first-slot sequence of every run; pairs: the (up to two) sequences of every run -> (first-slot deviation, inclusion
    deviation) in sigma, against the toy model's exact probabilities."""
    table = toy_sequences()
    seqs = sorted(table)
    p = np.array([table[s] for s in seqs])
    n = len(firsts)
    c1 = np.array([sum(1 for f in firsts if f == s) for s in seqs])
    c2 = np.array([sum(1 for pr in pairs if s in pr) for s in seqs])
    return sigma_deviation(c1, n, p), sigma_deviation(c2, n, inclusion_w2(p))


SIGMA_BOUND = 5.0


# ---------------------------------------------------------------------------------------------------------------------
# The checks shared by the tests of the reference and of the kernel.  Each takes a `step(logits, noise, state, t) -> state` function.
# ---------------------------------------------------------------------------------------------------------------------
def tie_case():
    """Slots 1 and 3 finished with EQUAL keys above everything else, slot 0 live, slot 2 empty; W = 4, V = 6."""
    state, _ = start_state(1, 4, TOY_L)
    state["gum"][0] = [-1.0, -0.5, NEG, -0.5]
    state["phi"][0] = [-2.0, -3.0, NEG, -4.0]
    state["fin"][0] = [False, True, False, True]
    state["len"][0] = [2, 2, 0, 2]
    state["tokens"][0, :, 1] = [4, SEP, 0, SEP]
    state["tokens"][0, 2] = 0
    rs = np.random.RandomState(3)
    return rs.randn(1, 4, TOY_V), rs.gumbel(size=(1, 4, TOY_V)), state, 2


def check_tie_order(step):
    """Two finished slots with equal keys keep their slot order; fewer finite candidates than W leaves the trailing slots empty."""
    lg, nz, state, t = tie_case()
    out = step(lg, nz, state, t)
    assert list(np.asarray(out["parent"])[0, :2]) == [1, 3], np.asarray(out["parent"])[0]
    assert list(np.asarray(out["phi"])[0, :2]) == [-3.0, -4.0]
    lg[0, 0, :] = MASKED
    lg[0, 0, 4] = 0.3                                                     # slot 0 has one allowed token: 3 finite candidates for 4 slots
    out = step(lg, nz, state, t)
    gum = np.asarray(out["gum"])[0]
    assert list(np.asarray(out["parent"])[0, :3]) == [1, 3, 0] and gum[2] == -1.0 and gum[3] == NEG and np.asarray(out["phi"])[0, 3] == NEG
    assert not np.asarray(out["fin"])[0, 3] and np.asarray(out["ids"])[3] == 0 and int(np.asarray(out["open"])[0]) == 1
