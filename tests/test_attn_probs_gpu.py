"""spmm_attn_probs (csrc/attnmap.hip) against float64 on the same bf16 inputs (tests/attn_map_reference.probs), at the smallest shapes at
which each mechanism can go wrong: one key, one tile, a tile boundary on either side, every key-tile count of the two published
directions (54 keys, 54 queries), 256 on either side, more than one query tile, 1 / 2 / 3 / 12 / 16 heads, packed rows over shared
sources, Q / K as column blocks of fused projection buffers, ldp > Lkv.

Tolerance.  The kernel's only error sources are the fp32 accumulation of 64 exact bf16 products and the fp32 exponential: of the order
1e-6 on a probability for randn inputs.  Measured on an MI355X, largest |kernel - float64| over every case below (head mean and per head):
1.197e-7 (per head, 12 heads x 54 x 128; head mean at most 5.4e-8).  The absolute tolerance is 4 x that, rounded: KERNEL_TOL = 4.8e-7,
below the 1e-4 above which a bf16-rounded numerator (2e-3 relative) would pass; tests/test_attention_maps_cpu.py shows that the six
seeded defects stay above 1e-4.  Every figure is printed before it is asserted.
Row sums: within 1e-5 of 1 -- at most 256 fp32 additions of values at most 1 (derived, not measured)."""
import pytest
import torch

import attn_map_reference as A

pytestmark = pytest.mark.gpu

CASES = A.kernel_cases()
NAMES = [c["name"] for c in CASES]
BF = torch.bfloat16


def _d(t):
    return None if t is None else t.cuda()


def _run(c, mean=True, heads=True, guard=2):
    """The launch of case c into NaN-filled outputs with `guard` rows around them.  -> (P_mean [rows, ldp] or None, P_heads [nH, rows, ldp]
    or None, the guarded buffers of both)."""
    from spmm_amd import ops
    H = c["nH"] * 64
    Q = c["Qbuf"].to(BF).cuda()[:, c["qcol"]:c["qcol"] + H]
    K = c["Kbuf"].to(BF).cuda()[:, c["kcol"]:c["kcol"] + H]
    lay = A.case_layout(c)
    rows, ldp = Q.shape[0], c["ldp"]
    bm = torch.full((rows + 2 * guard, ldp), float("nan"), device="cuda") if mean else None
    bh = torch.full((c["nH"], rows + 2 * guard, ldp), float("nan"), device="cuda") if heads else None
    kw = {k: (_d(v) if torch.is_tensor(v) else v) for k, v in lay.items()}
    ops.attn_probs(Q, K, P_mean=None if bm is None else bm[guard:guard + rows], P_heads=None if bh is None else bh[:, guard:guard + rows],
                   mean=mean, heads=heads, **kw)
    torch.cuda.synchronize()
    return (None if bm is None else bm[guard:guard + rows].cpu(), None if bh is None else bh[:, guard:guard + rows].cpu(),
            None if bm is None else bm.cpu(), None if bh is None else bh.cpu())


@pytest.fixture(scope="module")
def refs():
    """The float64 reference of every case, computed once and left unchanged."""
    return {c["name"]: A.probs(*A.case_qk(c), **A.case_layout(c)) for c in CASES}


@pytest.fixture(scope="module")
def runs():
    return {c["name"]: _run(c) for c in CASES}


def test_the_tolerance_is_below_the_ceiling():
    assert A.KERNEL_TOL == 4 * A.KERNEL_DEV_MEASURED and A.KERNEL_TOL < A.TOL_CEILING


@pytest.mark.parametrize("name", NAMES)
def test_probabilities_match_float64(name, refs, runs):
    c, ref = CASES[NAMES.index(name)], refs[name]
    pm, ph, bm, bh = runs[name]
    Lkv, o, keys = c["Lkv"], ref["owned"], ref["keys"]
    dm = (pm[o, :Lkv].double() - ref["mean"][o]).abs().max().item()
    dh = (ph[:, o, :Lkv].double() - ref["heads"][:, o]).abs().max().item()
    rs = pm[o, :Lkv].double().sum(1)
    alive = keys[o].any(1)
    print(f"[attn_probs] {name}: |kernel - float64| head mean {dm:.3e}, per head {dh:.3e} (tolerance {A.KERNEL_TOL:.2e}); "
          f"row sums within {(rs[alive] - 1).abs().max().item() if bool(alive.any()) else 0.0:.2e} of 1")
    assert dm <= A.KERNEL_TOL and dh <= A.KERNEL_TOL, (name, dm, dh)
    # masked columns are exactly 0 (also in every head); a row with every key masked is zeros
    assert bool((pm[o, :Lkv][~keys[o]] == 0).all()) and bool((ph[:, o, :Lkv][:, ~keys[o]] == 0).all())
    assert bool((pm[o, :Lkv][~alive] == 0).all())
    assert bool(((rs[alive] - 1).abs() <= 1e-5).all())
    hs = ph[:, o, :Lkv].double().sum(2)
    assert bool(((hs[:, alive] - 1).abs() <= 1e-5).all())
    # what is not written keeps its NaN fill: columns at Lkv and beyond, rows of no sequence, the guard rows around the outputs
    for buf in (bm, bh):
        inner = buf[..., 2:-2, :]
        assert bool(torch.isnan(buf[..., :2, :]).all()) and bool(torch.isnan(buf[..., -2:, :]).all())
        assert bool(torch.isnan(inner[..., Lkv:]).all())
        assert bool(torch.isnan(inner[..., ~o, :]).all())
        assert not bool(torch.isnan(inner[..., o, :Lkv]).any())


def test_the_all_masked_case_has_such_a_row(refs):
    ref = refs["dense-allmasked"]
    assert bool((~ref["keys"][ref["owned"]].any(1)).any())


@pytest.mark.parametrize("name", ["dense-2x2x17x15", "dense-2x12x54x128", "dense-2x2x130x129", "dense-allmasked", "packed-shared", "packed-text"])
def test_one_output_alone_gives_the_same_bits(name, runs):
    c = CASES[NAMES.index(name)]
    pm, ph, _, _ = runs[name]
    pm1, _, _, _ = _run(c, heads=False)
    _, ph1, _, _ = _run(c, mean=False)
    assert torch.equal(pm1.view(torch.int32), pm.view(torch.int32))
    assert torch.equal(ph1.view(torch.int32), ph.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- determinism
def _one(Q, K, *, nH, Lq, Lkv, **kw):
    from spmm_amd import ops
    pm, ph = ops.attn_probs(Q, K, nH=nH, Lq=Lq, Lkv=Lkv, mean=True, heads=True, **kw)
    torch.cuda.synchronize()
    return pm, ph


def test_a_sequence_has_the_same_bits_in_every_situation():
    """One sequence of 20 query rows over its 54-key source: alone; first, middle and last among other sequences; with launch Lkv of 54,
    64, 128 and 256; through kv_seq against a private copy of the source; dense against packed."""
    g = torch.Generator().manual_seed(8)
    nH, H, Lq, Ls = 2, 128, 20, 54
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")                                          # noqa: E731
    q, k = A._bf((Lq, H), g).to(BF).cuda(), A._bf((Ls, H), g).to(BF).cuda()
    oq, ok_ = [A._bf((Lq, H), g).to(BF).cuda() for _ in range(2)], [A._bf((Ls, H), g).to(BF).cuda() for _ in range(2)]
    pm0, ph0 = _one(q, k, nseq=1, nH=nH, Lq=Lq, Lkv=Ls)
    same = lambda pm, ph, r0: (torch.equal(pm[r0:r0 + Lq, :Ls].view(torch.int32), pm0.view(torch.int32))                # noqa: E731
                               and torch.equal(ph[:, r0:r0 + Lq, :Ls].view(torch.int32), ph0.view(torch.int32)))
    # dense, first / middle / last of three
    for pos in range(3):
        qs, ks = list(oq), list(ok_)
        qs.insert(pos, q)
        ks.insert(pos, k)
        pm, ph = _one(torch.cat(qs), torch.cat(ks), nseq=3, nH=nH, Lq=Lq, Lkv=Ls)
        assert same(pm, ph, pos * Lq), f"dense, position {pos}"
    # packed with a launch Lkv at and above the source's length; the others' sources are longer or shorter
    for Lkv in (54, 64, 128, 256):
        o_len = min(Lkv, 77)
        kk = torch.cat([A._bf((o_len, H), g).to(BF).cuda(), k, A._bf((3, H), g).to(BF).cuda()])
        qq = torch.cat([oq[0][:7], q, oq[1]])
        pm, ph = _one(qq, kk, nseq=3, nH=nH, Lq=Lq, Lkv=Lkv, q_row0=i32([0, 7, 7 + Lq]), q_len=i32([7, Lq, Lq]),
                      kv_row0=i32([0, o_len, o_len + Ls]), kv_len=i32([o_len, Ls, 3]))
        assert same(pm, ph, 7), f"packed, launch Lkv {Lkv}"
        assert bool((pm[7:7 + Lq, Ls:] == 0).all())
    # dense rows under a key mask of 54 in a launch of 128 keys
    km = torch.zeros(1, 128, dtype=torch.int32, device="cuda")
    km[:, :Ls] = 1
    pm, ph = _one(q, torch.cat([k, A._bf((128 - Ls, H), g).to(BF).cuda()]), nseq=1, nH=nH, Lq=Lq, Lkv=128, kmask=km)
    assert same(pm, ph, 0), "dense under kmask, launch Lkv 128"
    # through kv_seq (three query sequences share source 1 of 2) against a private copy per query sequence
    qq = torch.cat([oq[0], q, oq[1]])
    pm_s, ph_s = _one(qq, torch.cat([ok_[0], k]), nseq=3, nH=nH, Lq=Lq, Lkv=Ls, kv_seq=i32([1, 1, 0]))
    pm_p, ph_p = _one(qq, torch.cat([k, k, ok_[0]]), nseq=3, nH=nH, Lq=Lq, Lkv=Ls)
    assert same(pm_s, ph_s, Lq) and torch.equal(pm_s.view(torch.int32), pm_p.view(torch.int32)) and torch.equal(ph_s.view(torch.int32), ph_p.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- the trusted kernel
@pytest.mark.parametrize("name", A.AGREE_CASES)
def test_probabilities_times_v_agree_with_the_attention_kernel(name, runs):
    """P_heads @ V (fp32, torch) against ops.attn_fwd(is_cross=True, dropout_p=0) on the same launch layout, within the tolerances
    tests/test_kernels_gpu.py::test_attention_forward holds that kernel to (atol 1.5e-2, rtol 1e-2): the new kernel's mask and layout
    semantics are those of the trusted one."""
    from spmm_amd import ops
    c = CASES[NAMES.index(name)]
    nH, H, Lkv = c["nH"], c["nH"] * 64, c["Lkv"]
    Q = c["Qbuf"].to(BF).cuda()[:, c["qcol"]:c["qcol"] + H]
    K = c["Kbuf"].to(BF).cuda()[:, c["kcol"]:c["kcol"] + H]
    V = c["V"].to(BF).cuda()
    lay = {k: (_d(v) if torch.is_tensor(v) else v) for k, v in A.case_layout(c).items()}
    Oo = torch.zeros(Q.shape[0], H, dtype=BF, device="cuda")
    ops.attn_fwd(Q, K, V, Oo, None, is_cross=True, dropout_p=0.0, **lay)
    torch.cuda.synchronize()
    _, ph, _, _ = runs[name]
    ref = A.probs(*A.case_qk(c), **A.case_layout(c))
    want = torch.zeros(Q.shape[0], H)
    Vf = c["V"]
    for s in range(c["nseq"]):
        u = int(c["kv_seq"][s]) if c["kv_seq"] is not None else s
        nq = int(c["q_len"][s]) if c["q_len"] is not None else c["Lq"]
        r0 = int(c["q_row0"][s]) if c["q_row0"] is not None else s * c["Lq"]
        nk = int(c["kv_len"][u]) if c["kv_len"] is not None else Lkv
        k0 = int(c["kv_row0"][u]) if c["kv_row0"] is not None else u * Lkv
        for h in range(nH):
            want[r0:r0 + nq, h * 64:(h + 1) * 64] = ph[h, r0:r0 + nq, :nk] @ Vf[k0:k0 + nk, h * 64:(h + 1) * 64]
    o = ref["owned"]
    got = Oo.float().cpu()
    d = (got[o] - want[o]).abs()
    print(f"[attn_probs] {name}: |attn_fwd - P_heads @ V| max {d.max().item():.3e}")
    assert bool((d <= 1.5e-2 + 1e-2 * want[o].abs()).all()), d.max().item()
