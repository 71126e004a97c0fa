"""tests/decode_attn_reference.py checked on the CPU, at every problem tests/test_decode_attn_edges_gpu.py runs: the reference is the formula
the older kernel tests compare with; the case lists hold what they are meant to hold (all 24 instantiations of the grouped kernel, the
virtual-key counts, the parting positions, every key-identity premise); the buffers address the cells the launch arguments name and poison
the rest; a Python model of the kernels' walk passes check_output on every case, and the same model with any one of seven defects -- last
virtual key dropped, per-beam keys shown to the next beam, position s read as shared, no rescale at a new maximum, the newest key read from
the cache, rowmap ignored by the copy, t_ptr ignored -- is rejected wherever the defect applies.  So the GPU tests cannot pass a kernel that
drops, doubles or mis-attributes one key.  spmm_decode_attn's argument checks are exercised without a launch."""
import os

import pytest
import torch

import decode_attn_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [p.name for p in D.ALL_CASES]


@pytest.mark.parametrize("R,nH,Lkv,Lmax,kv_div,group", [(10, 2, 1, 16, 0, 1), (15, 12, 37, 64, 0, 5), (20, 12, 54, 54, 5, 5), (64, 4, 130, 160, 0, 4),
                                                    (6, 2, 256, 256, 3, 3), (35, 12, 9, 16, 0, 7), (12, 4, 70, 80, 0, 2), (18, 2, 33, 40, 0, 6),
                                                    (500, 12, 100, 100, 0, 5), (12, 2, 54, 54, 6, 6), (12, 2, 200, 256, 0, 6), (16, 2, 40, 48, 0, 8),
                                                    (16, 2, 54, 54, 8, 8), (10, 3, 17, 32, 0, 5)])
def test_reference_is_the_formula_of_the_kernel_test(R, nH, Lkv, Lmax, kv_div, group):
    """attention() in float64 and float32 against the fp32 torch lines of test_kernels_gpu.py::test_decode_attention_over_kv_cache, on that
    test's shapes and data (the first 40 rows of the 500-row shape), and A >= |out|."""
    H = nH * 64
    g = torch.Generator().manual_seed(R + Lkv)
    q = torch.randn(R, 3 * H, generator=g).to(D.BF)
    nseq = R if kv_div == 0 else (R + kv_div - 1) // kv_div
    wide = 2 * H if kv_div else H
    cache = torch.randn(nseq, Lmax, wide, generator=g).to(D.BF)
    Kc = cache[:, :, :H]
    Vc = cache[:, :, H:] if kv_div else torch.randn(nseq, Lmax, H, generator=g).to(D.BF)
    anc = None if kv_div else torch.randint(0, R, (R, Lmax), generator=g)
    n = min(R, 40)
    j = torch.arange(Lkv)
    seq = (anc[:, :Lkv] if kv_div == 0 else (torch.arange(R) // kv_div)[:, None].expand(R, Lkv))[:n]
    K = Kc.float()[seq, j[None, :]].view(n, Lkv, nH, 64)
    V = Vc.float()[seq, j[None, :]].view(n, Lkv, nH, 64)
    s = torch.einsum("rhd,rjhd->rhj", q[:n, :H].float().view(n, nH, 64), K) * 0.125
    want = torch.einsum("rhj,rjhd->rhd", torch.softmax(s, -1), V)
    live = torch.ones(n, Lkv, dtype=torch.bool)
    got64, A, P = D.attention(q[:n, :H].view(n, nH, 64), K.to(D.BF), V.to(D.BF), live, torch.float64)
    got32 = D.attention(q[:n, :H].view(n, nH, 64), K.to(D.BF), V.to(D.BF), live, torch.float32)[0]
    assert got64.dtype == torch.float64 and got32.dtype == torch.float32
    assert (got64 - want.double()).abs().max().item() <= 2e-5 and (got32 - want).abs().max().item() <= 2e-5
    assert bool((A >= got64.abs() - 1e-12).all()) and bool(((P.sum(-1) - 1).abs() < 1e-12).all())
    # a masked key is as good as absent
    live[:, Lkv // 2:] = False
    half = D.attention(q[:n, :H].view(n, nH, 64), K.to(D.BF), V.to(D.BF), live, torch.float64)[0]
    if Lkv > 1:
        cut = D.attention(q[:n, :H].view(n, nH, 64), K[:, :Lkv // 2].to(D.BF), V[:, :Lkv // 2].to(D.BF), live[:, :Lkv // 2], torch.float64)[0]
        assert (half - cut).abs().max().item() <= 1e-12


def test_case_lists_hold_what_they_are_for():
    assert len(set(IDS)) == len(IDS) and set(D.FAMILIES) == {"instantiations", "parting", "nv", "lkv", "t_ptr", "new", "new_args", "same_args",
                                                             "per_row", "varlen", "grid", "extremes", "identity"}
    # all 24 instantiations of decode_attn_mfma_kernel<G, ALLSAME, VARLEN>, in the family meant for them and again with knew / vnew
    want = {(G, allsame, varlen) for G in range(1, 9) for (allsame, varlen) in ((True, False), (False, False), (True, True))}
    assert {D.instantiation(p) for p in D.CASES_INSTANTIATIONS} == want and len(want) == 24
    assert {(p.G, p.Lkv) for p in D.CASES_NEW} == {(G, L) for G in range(1, 9) for L in (1, 2, 17, 256)} and all(p.new and p.form == "anc" for p in D.CASES_NEW)
    assert {p.G for p in D.CASES_SAME_ARGS} == {1, 2, 4, 7} and 3 in {p.G for p in D.CASES_PARTING}
    # the virtual key counts, from the tables themselves; the hand-written table says the same
    for (G, L, s, nv), p in zip(D.NV_TABLE, D.CASES_NV):
        assert D.parting(p) == [(L if s is None else s, nv)] * p.nmol, p.name
    nvs = {nv for p in D.CASES_NV if p.form == "anc" for _, nv in D.parting(p)}
    assert nvs == set(D.NV_SET) == {p.Lkv for p in D.CASES_NV if p.form == "same"}
    assert {-(-nv // 16) for nv in nvs} == {1, 2, 3, 4}
    # a last block with ONE key, which only the last beam sees: empty for every other beam
    assert any(nv % 16 == 1 and nv > 16 and p.G > 1 for p in D.CASES_NV if p.form == "anc" for _, nv in D.parting(p))
    assert any(nv == 17 and p.G == 1 for p in D.CASES_NV if p.form == "anc" for _, nv in D.parting(p))       # ... and one where it is beam 0's
    # where ancestries part: every listed s, as the kernel derives it from the table, for G = 3 and G = 5
    for G in (3, 5):
        got = {D.parting(p)[0][0] for p in D.CASES_PARTING if p.G == G}
        assert got == {0, 15, 16, 17, 31, 32, 39, 40}, got
        assert all(p.Lkv == 40 and len(set(D.parting(p))) == 1 for p in D.CASES_PARTING)
    # Lkv and the device-side position
    assert [p.Lkv for p in D.CASES_LKV] == list(D.LKV_SET) + [256] and D.CASES_LKV[-1].G == 8 and D.parting(D.CASES_LKV[-1]) == [(0, 2048)] * 2
    assert [p.Leff for p in D.CASES_T_PTR] == list(D.LKV_SET) + [40] and all(p.Lkv == p.lmax for p in D.CASES_T_PTR[:-1])
    assert D.CASES_T_PTR[-1].t + 1 > D.CASES_T_PTR[-1].Lkv                               # clamps
    assert any(p.t is not None and p.new for p in D.CASES_NEW_ARGS) and any(p.rowmap and p.new for p in D.CASES_NEW_ARGS)
    assert any(p.layout == "head" and p.new for p in D.CASES_NEW_ARGS)
    assert {(p.layout, p.seq0) for p in D.CASES_SAME_ARGS} == {("fused", False), ("fused", True), ("wide", False), ("head", False)}
    # the per-row kernel is reached through group > 8 or kv_div != group alone
    assert all(not D.is_grouped(p) and (p.G > 8 or p.kv_div != p.G) for p in D.CASES_PER_ROW)
    tab = [p for p in D.CASES_PER_ROW if p.has_table]
    assert {p.G for p in tab} == {9, 12, 32} and {(p.new, p.t is not None) for p in tab if p.G == 32} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(p.new and p.t is not None and p.t > p.Lkv - 1 for p in tab)                 # j = min(*t_ptr, Lkv - 1)
    assert {1, 7, 8, 9, 256} <= {p.Lkv for p in tab} and {3, 4, 5} <= {p.R * p.nH for p in D.CASES_PER_ROW if not p.has_table}
    # variable-length memory
    assert {1, 15, 16, 17, 33} <= set(D.CASES_VARLEN[0].lens) and any(max(p.lens) > p.Lkv for p in D.CASES_VARLEN)
    assert any(p.kv_seq and len(set(p.kv_seq)) < len(p.kv_seq) and list(p.kv_seq) != sorted(p.kv_seq) for p in D.CASES_VARLEN)
    assert {p.nmol * p.nH for p in D.CASES_GRID} == {1, 7, 8, 9}
    # score extremes in the three forms; "ahead by more than 100" from the float64 scores
    for form in ("anc", "same", "per_row"):
        assert {p.score for p in D.CASES_EXTREMES if p.form == form} >= {"equal", "hot_first", "hot_last", "hot_tail", "zero_q"}
    for p in D.CASES_EXTREMES:
        lead = D.score_lead(p)
        if p.score.startswith("hot_"):
            assert bool((lead.reshape(p.nmol, -1) > 100).any(1).all()), (p.name, lead.max().item())
        elif p.score in ("equal", "zero_q") and p.Leff > 1:
            assert bool((lead == 0).all()), p.name
    hot = {p.score: D.world(p).hot[0, 0].item() for p in D.CASES_EXTREMES if p.form == "anc" and not p.new and p.score.startswith("hot_")}
    assert hot["hot_first"] < 16 and hot["hot_tail"] == 34 and hot["hot_last"] == 39      # first block, the first per-beam position, the last block
    # key identity: every (beam, position) is some row's hot key, in every problem; the premises are asserted by reference()
    for p in D.CASES_IDENTITY:
        w = D.world(p)
        D.reference(p)
        for u in set(w.src[:, 0].tolist()) if p.form == "varlen" else [None]:
            rows = torch.arange(p.R) if u is None else (w.src[:, 0] == u).nonzero()[:, 0]
            L = int(w.lens[rows[0]])
            seen = {(int(r) % p.G, int(w.hot[r, h])) for r in rows for h in range(p.nH)}
            assert seen == {(b, j) for b in range(p.G) for j in range(L)}, p.name
    idf = {(p.form, p.new, p.seq0, bool(p.kv_seq), p.rowmap) for p in D.CASES_IDENTITY}
    assert ("anc", False, False, False, False) in idf and ("anc", True, False, False, True) in idf and ("same", False, True, False, False) in idf
    assert ("varlen", False, False, True, False) in idf and any(f[0] == "per_row" for f in idf)
    # every defect applies somewhere
    for d in D.DEFECTS:
        assert sum(d in D.applicable_defects(p) for p in D.ALL_CASES) >= 8, d
    # what the entry points require of every buffer
    for p in D.ALL_CASES:
        s = D.launch_spec(p)
        assert p.ldq % 8 == 0 and p.ldo % 8 == 0 and (p.lmax >= p.Lkv or p.form == "varlen") and s.tok % 8 == 0 and s.hs >= 64
        assert 1 <= p.Lkv <= 256 and p.lmax <= 256 and D.world(p).total * 2 <= 1 << 24 and p.R * p.nH <= 800


@pytest.mark.parametrize("p", D.ALL_CASES, ids=IDS)
def test_buffers_poison_what_the_reference_does_not_read(p):
    """The cells the launch arguments name (s * seq_stride + j * tok_stride + h * head_stride + d behind K / V, through the ancestry table,
    r / kv_div or kv_row0 -- written out again here) hold what the reference reads; every other element of the key / value buffer is NaN;
    table entries past the end name the all-NaN row and nothing is out of range."""
    w, b, s = D.world(p), D.operand_buffers(p), D.launch_spec(p)
    K, V, live = D.gathered(p)
    R, nH = p.R, p.nH
    used = torch.zeros(w.total, dtype=torch.bool)
    d = torch.arange(64)
    for r in range(R):
        L = int(w.lens[r])
        for j in range(L):
            if p.new and j == L - 1:
                assert torch.equal(b.qkv[r, p.H:2 * p.H].view(nH, 64), K[r, j]) and torch.equal(b.qkv[r, 2 * p.H:3 * p.H].view(nH, 64), V[r, j])
                continue
            if p.form == "varlen":
                u = r // p.G if b.kv_seq is None else int(b.kv_seq[r // p.G])
                base = (int(b.row0[u]) + j) * s.tok
                assert j < int(b.kv_len[u])
            else:
                row = int(b.anc[r, j]) if b.anc is not None else r // s.kv_div
                base = row * s.seq_stride + j * s.tok
            for h in range(nH):
                at = base + h * s.hs + d
                assert torch.equal(b.kv[s.koff + at], K[r, j, h]) and torch.equal(b.kv[s.voff + at], V[r, j, h]), (r, j, h)
                used[s.koff + at] = True
                used[s.voff + at] = True
    assert bool(torch.isnan(b.kv[~used].float()).all()) and bool(torch.isfinite(b.kv[used].float()).all())
    assert torch.equal(b.qkv[:, :p.H].reshape(R, nH, 64), w.q) and bool(torch.isnan(b.qkv[:, -D.PAD_COLS:].float()).all())
    if b.anc is not None:
        assert int(b.anc.min()) >= 0 and int(b.anc.max()) < w.S and bool((b.anc[:, p.Leff:] == w.dead).all()) and b.anc.shape[1] >= p.Lkv
        dead = D.cell_index(w, torch.full((p.lmax,), w.dead), torch.arange(p.lmax))
        assert bool(torch.isnan(b.kv[s.koff + dead].float()).all()) and bool(torch.isnan(b.kv[s.voff + dead].float()).all())
    if p.rowmap:
        own = b.rowmap.tolist()
        assert len(set(own)) == R and own != sorted(own) and max(own) >= R and w.S > R + 1
        assert p.new and bool((b.anc[torch.arange(R), p.Leff - 1] == b.rowmap).all())
    if p.new:
        idx = D.cell_index(w, w.own, torch.full((R,), p.Leff - 1))
        assert bool(torch.isnan(b.kv[s.koff + idx].float()).all())                        # the launch fills these
        assert int((D._bits(D.expected_kv(p)) != D._bits(b.kv)).sum()) == 2 * R * nH * 64
    assert bool((D._bits(b.out) == D._bits(torch.tensor([D.SENTINEL], dtype=D.BF))).all())


@pytest.mark.parametrize("p", D.ALL_CASES, ids=IDS)
def test_model_of_the_walk_passes_and_every_applicable_defect_fails(p):
    ref64, A, ref32 = D.reference(p)
    b = D.operand_buffers(p)
    b.out[:p.R, :p.H] = ref32.to(D.BF)
    b.kv = D.expected_kv(p)
    D.check_output(f"{p.name} fp32 reference", b, p)
    D.check_output(f"{p.name} model", D.model(p), p)
    for d in D.applicable_defects(p):
        with pytest.raises(AssertionError):
            D.check_output(f"{p.name} {d}", D.model(p, d), p)


def test_check_output_guards_the_cells_around_the_views():
    p = D.CASES_NEW_ARGS[4]
    assert p.new and p.rowmap
    good = D.model(p)
    D.check_output(p.name, good, p)
    w = D.world(p)
    for what in ("pad_column", "row_R", "cache_cell", "cache_pad", "nan_out"):
        m = D.model(p)
        if what == "pad_column":
            m.out[0, p.H] = 1.0
        elif what == "row_R":
            m.out[p.R, 0] = 1.0
        elif what == "cache_cell":
            idx = D.cell_index(w, w.own[:1], torch.tensor([0]))                          # a 129th byte row: position 0 of an own row
            m.kv = m.kv.clone()
            m.kv[w.koff + idx] = 1.0
        elif what == "cache_pad":
            m.kv = m.kv.clone()
            m.kv[w.total - 1] = 0.0
        else:
            m.out[1, 3] = D.NAN
        with pytest.raises(AssertionError):
            D.check_output(f"{p.name} {what}", m, p)


# ----------------------------------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    return so


def _attn_args(**kw):
    a = dict(q=64, ldq=128, K=64, V=192, seq_stride=40 * 256, tok_stride=256, head_stride=64, anc=64, anc_ld=40, kv_div=1, group=3, out=64, ldo=128,
             R=6, nH=2, Lkv=37, scale=0.125, t_ptr=None, knew=None, vnew=None, ldn=0, rowmap=None)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_decode_attn_validates_its_arguments_without_touching_the_gpu(built):
    """Every refusal happens before the launch (the non-null pointers here are never dereferenced): the checks the entry point had, and the
    ones it shares with spmm_decode_xattn since this file -- 255 * tok_stride < 2^31 (the kernels form j * tok_stride in 32 bits), q, K, V,
    knew, vnew 16-byte aligned, out 8-byte aligned."""
    from spmm_amd._lib import lib
    L = lib()
    new = dict(knew=64, vnew=192, ldn=384)
    for kw, msg in ((dict(R=0), "R=0"), (dict(Lkv=0), "Lkv=0"), (dict(Lkv=257, anc_ld=300), "Lkv=257"), (dict(anc_ld=36), "anc_ld=36"),
                    (dict(anc=None, kv_div=0), "kv_div=0"), (dict(head_stride=56), "head_stride=56"), (dict(head_stride=68), "head_stride=68"),
                    (dict(seq_stride=40 * 256 + 4), "16-B alignment"), (dict(tok_stride=260), "16-B alignment"), (dict(ldq=120), "16-B alignment"),
                    (dict(ldo=64), "16-B alignment"), (dict(R=7), "multiple of group"), (dict(group=0), "group=0"),
                    (dict(knew=64), "come together"), (dict(anc=None, **new), "come together"), (dict(**{**new, "ldn": 64}), "ldn=64"),
                    (dict(**{**new, "ldn": 388}), "ldn=388"),
                    (dict(tok_stride=8421512), "tok_stride=8421512"), (dict(tok_stride=-256), "tok_stride=-256"),
                    (dict(q=72), "misaligned"), (dict(K=8), "misaligned"), (dict(V=200), "misaligned"), (dict(**{**new, "knew": 72}), "misaligned"),
                    (dict(**{**new, "vnew": 8}), "misaligned"), (dict(out=68), "misaligned"),
                    (dict(q=None), "are required"), (dict(K=None), "are required"), (dict(V=None), "are required"), (dict(out=None), "are required")):
        with pytest.raises(RuntimeError, match=msg):
            L.call("spmm_decode_attn", *_attn_args(**kw))
    assert 255 * 8421512 >= 2 ** 31 > 255 * 8421504                                      # the first tok_stride (a multiple of 8) that is refused
