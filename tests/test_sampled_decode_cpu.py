"""Host side of the seeded sampled PV -> SMILES search (spmm_amd/decode.py, pv2smiles.py): the counter hash and its Gumbel transform,
the Gumbel-top-k draw against the distribution it must have, the tensor-op candidate pick, the beam bookkeeping it feeds against a
sequential one-molecule search, and the driver's argument / condition plumbing.  No GPU."""
import importlib
import math

import numpy as np
import pytest
import torch

from spmm_amd import decode

CLS, SEP = decode.CLS_ID, decode.SEP_ID


# ---- an independent restatement of csrc/common.h: mix32 / splitmix64 / seed_mix / rng_pair, one element at a time on Python integers
def _mix32(x):
    x ^= x >> 16; x = x * 0x21f0aaad & 0xffffffff
    x ^= x >> 15; x = x * 0x735a2d97 & 0xffffffff
    return x ^ (x >> 15)


def _sm64(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & m
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & m
    return z ^ (z >> 31)


def _rng_pair(seed, idx):
    lo, hi, s0, s1 = idx & 0xffffffff, idx >> 32, seed & 0xffffffff, seed >> 32
    return _mix32(((lo ^ s0) + (hi ^ s1) * 0x9E3779B1) & 0xffffffff)


@pytest.mark.parametrize("seed,salt,mols,t,k,V,Lmax", [(1234, 77, [0, 1, 5], 3, 2, 7, 19), (2 ** 63 + 11, 0x50563253, [3, 70000, 2 ** 31 + 5], 102, 5, 11, 103),
                                                      (0, 0, [0], 0, 1, 3, 4)])
def test_host_noise_is_the_counter_hash(seed, salt, mols, t, k, V, Lmax):
    """gumbel_bits_host gives, element by element, rng_pair(seed_mix(seed, salt), (((mol * Lmax + t) * k + b) * V + j)) >> 8 -- 64-bit
    counters included (molecule 2^31 + 5 at Lmax 103 passes 2^32) -- and gumbel_noise_host is -log(-log((x + 0.5) 2^-24)) of it."""
    bits = decode.gumbel_bits_host(seed, salt, mols, t, k, V, Lmax)
    assert bits.shape == (len(mols), k, V) and bits.dtype == np.int64
    key = _sm64((_sm64(seed & (2 ** 64 - 1)) + salt) & (2 ** 64 - 1))
    for a, mol in enumerate(mols):
        for b in range(k):
            for j in range(V):
                idx = (((mol * Lmax + t) * k + b) * V + j) & (2 ** 64 - 1)
                assert int(bits[a, b, j]) == _rng_pair(key, idx) >> 8, (mol, b, j)
    g = decode.gumbel_noise_host(seed, salt, mols, t, k, V, Lmax)
    assert g.dtype == torch.float64 and tuple(g.shape) == (len(mols) * k, V)
    want = [-math.log(-math.log((int(x) + 0.5) * 2.0 ** -24)) for x in bits.reshape(-1)]
    torch.testing.assert_close(g.reshape(-1), torch.tensor(want, dtype=torch.float64), rtol=0, atol=1e-12)      # (two libms: the last bit of a float64 log)


def test_uniforms_lie_strictly_inside_the_unit_interval():
    bits = decode.gumbel_bits_host(9, 1, range(3000), 2, 2, 50, 19)
    assert bits.min() >= 0 and bits.max() < 2 ** 24
    for x in (0, 2 ** 24 - 1, int(bits.min()), int(bits.max())):         # the ends of the range too, whether or not this draw reached them
        u = (x + 0.5) * 2.0 ** -24
        assert 0.0 < u < 1.0 and math.isfinite(-math.log(-math.log(u)))
    assert torch.isfinite(decode.gumbel_noise_host(9, 1, range(3000), 2, 2, 50, 19)).all()


def test_gumbel_top_k_draws_pairs_without_replacement_from_the_softmax():
    """k = 2 draws of beam 1 at positions 1 and 5 for 40 000 molecules: the frequency of every ORDERED pair (i, j) against
    p_i p_j / (1 - p_i) -- what torch.multinomial(p, 2, replacement=False) has, in draw order.  |z| < 4 in each of the 2 x 42 = 84 cells
    (a standard normal passes 4 with probability 6e-5 per cell).  A failure is a finding about the hash, not a reason to change the seed."""
    V, k, Lmax, M = 7, 2, 19, 40000
    logits = torch.tensor([1.2, 0.3, -0.5, 2.0, 0.0, -1.0, 0.7])
    p = torch.softmax(logits.double(), 0)
    worst = 0.0
    for t in (1, 5):
        noise = decode.gumbel_noise_host(1234, 77, range(M), t, k, V, Lmax).view(M, k, V)[:, 1]
        _, ids = decode._pick_seeded(logits.expand(M, V), noise, k)
        count = torch.zeros(V, V, dtype=torch.long)
        count.index_put_((ids[:, 0], ids[:, 1]), torch.ones(M, dtype=torch.long), accumulate=True)
        assert int(count.diagonal().sum()) == 0                          # without replacement
        for i in range(V):
            for j in range(V):
                if i != j:
                    q = float(p[i] * p[j] / (1 - p[i]))
                    z = (int(count[i, j]) - M * q) / math.sqrt(M * q * (1 - q))
                    worst = max(worst, abs(z))
                    assert abs(z) < 4, (t, i, j, int(count[i, j]), M * q, z)
    print(f"Gumbel-top-2 pair frequencies: worst |z| over 84 cells {worst:.2f}")


def test_pick_seeded_returns_unperturbed_log_probs_in_descending_key_order():
    g = torch.Generator().manual_seed(3)
    logits, noise = torch.randn(4, 3, 20, generator=g) * 2, torch.randn(4, 3, 20, generator=g) * 3
    k = 5
    lp, ids = decode._pick_seeded(logits, noise.reshape(12, 20), k)
    assert tuple(lp.shape) == (4, 3, k) and tuple(ids.shape) == (4, 3, k)
    key = logits + noise
    picked = key.gather(-1, ids)
    assert bool((picked[..., :-1] > picked[..., 1:]).all())              # descending keys
    rest = key.scatter(-1, ids, -float("inf")).max(-1).values
    assert bool((picked[..., -1] > rest).all())                          # and they are the k largest
    assert torch.equal(lp, torch.log_softmax(logits, -1).gather(-1, ids))
    assert not torch.equal(ids, torch.topk(logits, k, -1).indices)       # (the noise did change the pick)
    # zero noise: the deterministic pick
    lp0, ids0 = decode._pick_seeded(logits, torch.zeros(12, 20), k)
    assert torch.equal(ids0, torch.topk(logits, k, -1).indices)


def _sequential_search(first_logits, step_logits, noise0, step_noise, k):
    """The reference's one-molecule search (d_pv2smiles_single.py:79-103) with the candidates of every beam taken by Gumbel-top-k from
    the given noise.  first_logits [V], step_logits [T, k, V], noise0 [V], step_noise [T, k, V] -> [(score, tokens)] best first."""
    def pick(lg, nz):
        ids = torch.argsort(lg + nz, descending=True, stable=True)[:k]
        return torch.log_softmax(lg, -1)[ids], ids

    cur, ids = pick(first_logits, noise0)
    seqs = [[CLS, int(i)] for i in ids]
    finals = []
    for s in range(step_logits.shape[0]):
        picks = [pick(step_logits[s, b], step_noise[s, b]) for b in range(k)]
        k2 = torch.stack([cur[b] + picks[b][0] for b in range(k)])
        tok = torch.stack([picks[b][1] for b in range(k)])
        for b in range(k):
            for r in range(k):
                if int(tok[b, r]) == SEP:
                    finals.append((float(k2[b, r]), seqs[b] + [SEP]))
                    k2[b, r] = -1e5
        if len(finals) >= k:
            break
        cur, flat = torch.topk(k2.flatten(), k)
        seqs = [seqs[int(f) // k] + [int(tok[int(f) // k, int(f) % k])] for f in flat]
    order = sorted(range(len(finals)), key=lambda i: -finals[i][0])      # (stable)
    return [finals[i] for i in order[:k]]


@pytest.mark.parametrize("N,k,V,T", [(12, 3, 30, 10), (5, 1, 9, 12), (7, 4, 40, 8)])
def test_seeded_pick_feeds_the_batched_bookkeeping_like_a_sequential_search(N, k, V, T):
    """BeamBook.update fed by _pick_seeded for N molecules at once against the sequential search of each molecule, from the same
    counter noise (position 0: t = 0, b = 0; position s + 1: t = s + 1): same finals in the same order, scores within 1e-5."""
    Lmax, seed, base = T + 3, 21, 100
    g = torch.Generator().manual_seed(N * k + V)
    first = torch.randn(N, V, generator=g) * 2
    steps = torch.randn(T, N, k, V, generator=g) * 2
    steps[..., SEP] += torch.where(torch.rand(T, N, k, generator=g) < 0.25, 5.0, -2.0)
    mols = range(base, base + N)
    nz = [decode.gumbel_noise_host(seed, decode.GUMBEL_SALT, mols, t, k, V, Lmax).float() for t in range(T + 1)]
    book = decode.BeamBook(N, k, T, "cpu")
    book.first(*decode._pick_seeded(first, nz[0].view(N, k, V)[:, 0], k))
    for s in range(T):
        book.update(*decode._pick_seeded(steps[s], nz[s + 1], k))
    got = book.results()
    n_fin = 0
    for n in range(N):
        want = _sequential_search(first[n], steps[:, n], nz[0].view(N, k, V)[n, 0], torch.stack([z.view(N, k, V)[n] for z in nz[1:]]), k)
        assert [h[1] for h in got[n]] == [h[1] for h in want], n
        for (pa, _), (pb, _) in zip(got[n], want):
            assert abs(pa - pb) < 1e-5
        n_fin += len(want)
    assert n_fin >= N // 2                                               # the scenario does finish hypotheses


def test_new_ops_match_the_header_prototypes():
    """ops.gumbel_noise and ops.beam_step(noise=...) against include/spmm_hip.h, argument by argument, without a launch."""
    from spmm_amd import ops
    N, k, V, T = 3, 2, 30, 5
    book = decode.BeamBook(N, k, T, "cpu", fused=True)
    ops._DRY_RUN, ops._dry_log[:] = True, []
    try:
        seed = torch.tensor([5], dtype=torch.int64)
        noise = ops.gumbel_noise(seed, N, k, V, T + 3, salt=decode.GUMBEL_SALT, t=1, mol_base=7)
        assert tuple(noise.shape) == (N * k, V) and noise.dtype == torch.float32
        ops.beam_step(torch.zeros(N * k, V), book, t=2, noise=noise)
        ops.beam_step(torch.zeros(N * k, V), book, t=2)
        assert ops._dry_log == ["spmm_gumbel_noise", "spmm_beam_step_sampled", "spmm_beam_step"]
    finally:
        ops._DRY_RUN = False


# ---- the driver
def test_driver_flags_and_defaults():
    drv = importlib.import_module("pv2smiles")
    a = drv.parse_args([])
    # the reference's flags and defaults (d_pv2smiles_single.py:227-233)
    assert (a.checkpoint, a.vocab_filename, a.device, a.n_generate, a.k, a.stochastic) == \
        ("./Pretrain/checkpoint_SPMM.ckpt", "./vocab_bpe_300.txt", "cuda", 1000, 2, True)
    assert (a.seed, a.input, a.property_names, a.normalize, a.output, a.synthetic, a.tiny) == (0, "", "", "", "generated_molecules.txt", False, False)
    b = drv.parse_args(["--synthetic", "--tiny", "--n_generate", "8", "--seed", "1", "--stochastic", "False", "--k", "3", "--output", "x.txt"])
    assert b.synthetic and b.tiny and b.n_generate == 8 and b.seed == 1 and b.stochastic is False and b.k == 3 and b.output == "x.txt"


def test_driver_maps_the_input_csv_onto_pv_and_mask(tmp_path):
    drv = importlib.import_module("pv2smiles")
    names = [f"P{i}" for i in range(53)]
    names[14], names[50] = "MolWt", "QED"
    (tmp_path / "names.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "in.csv").write_text("property,input_value\nQED,0.8\nMolWt,150\n")
    pv, mask = drv.read_condition(str(tmp_path / "in.csv"), str(tmp_path / "names.txt"))
    assert tuple(pv.shape) == (53,) and tuple(mask.shape) == (53,)
    want_pv, want_mask = torch.zeros(53), torch.ones(53)
    want_pv[14], want_pv[50] = 150.0, 0.8
    want_mask[14] = want_mask[50] = 0
    assert torch.equal(pv, want_pv) and torch.equal(mask, want_mask)
    (tmp_path / "bad.csv").write_text("property,input_value\nNoSuch,1\n")
    with pytest.raises(SystemExit):
        drv.read_condition(str(tmp_path / "bad.csv"), str(tmp_path / "names.txt"))
    np.savez(tmp_path / "norm.npz", mean=np.arange(53, dtype=np.float32), std=np.full(53, 2.0, dtype=np.float32))
    mean, std = drv.read_normalize(str(tmp_path / "norm.npz"))
    assert torch.equal(mean, torch.arange(53.0)) and torch.equal(std, torch.full((53,), 2.0))
    vocab = drv.synthetic_vocab(300)
    assert len(vocab) == 300 == len(set(vocab)) and vocab[:4] == ["[PAD]", "[UNK]", "[CLS]", "[SEP]"]
