"""Per-kernel parity of the two entry points reaction prediction adds (through the C ABI): spmm_decode_xattn -- single-query cross-attention
over a masked, variable-length memory -- against fp32 torch on the same bf16 inputs (tolerance of test_decode_attention_over_kv_cache:
2e-2 absolute + 2e-2 relative), and spmm_beam_step_until against the tensor-op bookkeeping BeamBook(need=...)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LENS = [1, 2, 15, 16, 17, 31, 32, 33, 48, 149, 255, 256]          # straddle every 16-key block and both slots of the ring


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops as o
    return o


def close(got, ref, atol, rtol, name=""):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())                       # (a NaN is bad)
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} off; max err {err.max().item():.4g} first bad idx {bad.nonzero()[0].tolist()}"


def reference(q, K, V, row0, lens, seq, group, nH):
    """fp32 torch on the same bf16 inputs: row r of molecule n = r // group attends rows row0[u] .. + lens[u] - 1 of K / V, u = seq[n]."""
    R = q.shape[0]
    out = torch.empty(R, nH * 64, dtype=torch.float32, device=q.device)
    for n in range(R // group):
        u = int(seq[n])
        a, L = int(row0[u]), int(lens[u])
        k = K[a:a + L].float().view(L, nH, 64)
        v = V[a:a + L].float().view(L, nH, 64)
        qq = q[n * group:(n + 1) * group].float().view(group, nH, 64)
        s = torch.einsum("ghd,jhd->ghj", qq, k) * 0.125
        out[n * group:(n + 1) * group] = torch.einsum("ghj,jhd->ghd", torch.softmax(s, -1), v).reshape(group, nH * 64)
    return out


def packed(lens, order, H, seed, pad_rows=0, fill=None):
    """A packed [M, 2H] key|value buffer holding the sources in `order`, as a view of a larger tensor: -> (KV, row0 int32, lens int32)."""
    g = torch.Generator().manual_seed(seed)
    M = sum(lens)
    big = torch.randn(M + pad_rows, 2 * H, generator=g).to(BF)
    if fill is not None:
        big[M:] = fill
    row0 = [0] * len(lens)
    at = 0
    for u in order:
        row0[u] = at
        at += lens[u]
    return big.cuda()[:M], torch.tensor(row0, dtype=torch.int32).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()


@pytest.fixture(scope="module")
def twelve():
    """The 12-length case, built once: packed rows in a shuffled source order, queries for up to 8 beams per source."""
    nH, H = 2, 128
    order = torch.randperm(len(LENS), generator=torch.Generator().manual_seed(1)).tolist()
    KV, row0, lens = packed(LENS, order, H, seed=2)
    q = torch.randn(len(LENS) * 8, 3 * H, generator=torch.Generator().manual_seed(3)).to(BF).cuda()      # strided view like a fused projection
    return nH, H, KV, row0, lens, q


@pytest.mark.parametrize("group", [1, 2, 5, 8])
def test_variable_lengths_in_one_launch(ops, twelve, group):
    nH, H, KV, row0, lens, q = twelve
    U = len(LENS)
    qq = q[:U * group, :H]
    out = torch.zeros(U * group, H, dtype=BF, device="cuda")
    ops.decode_xattn(qq, KV[:, :H], KV[:, H:], out, nH=nH, kv_row0=row0, kv_len=lens, Lkv_max=256, group=group)
    ref = reference(qq, KV[:, :H], KV[:, H:], row0.tolist(), LENS, list(range(U)), group, nH)
    close(out, ref, 2e-2, 2e-2, f"decode_xattn group {group}")
    # repeat stability: the ring is fed by LDS-DMA behind counted waits -- every launch must give the same bits
    again = torch.zeros_like(out)
    ops.decode_xattn(qq, KV[:, :H], KV[:, H:], again, nH=nH, kv_row0=row0, kv_len=lens, Lkv_max=256, group=group)
    assert torch.equal(out, again)


@pytest.mark.parametrize("group", [1, 2, 5, 8])
def test_molecules_mapped_onto_sources(ops, group):
    """kv_seq: 7 molecules on 3 sources, one source repeated, out of order."""
    nH, H = 2, 128
    lens = [17, 149, 33]
    KV, row0, lens_d = packed(lens, [2, 0, 1], H, seed=5)
    seq = [2, 0, 0, 1, 2, 1, 0]
    kv_seq = torch.tensor(seq, dtype=torch.int32).cuda()
    q = torch.randn(7 * group, H, generator=torch.Generator().manual_seed(6)).to(BF).cuda()
    out = torch.zeros(7 * group, H, dtype=BF, device="cuda")
    ops.decode_xattn(q, KV[:, :H], KV[:, H:], out, nH=nH, kv_seq=kv_seq, kv_row0=row0, kv_len=lens_d, Lkv_max=149, group=group)
    close(out, reference(q, KV[:, :H], KV[:, H:], row0.tolist(), lens, seq, group, nH), 2e-2, 2e-2, f"decode_xattn kv_seq group {group}")


def test_masked_rows_are_not_used(ops):
    """Padded layout [U, 64, 2H] (kv_row0[u] = 64 u) with every row at or beyond a source's length NaN, and a packed layout whose last source
    ends exactly at the buffer's last row, the buffer a view into a larger NaN-filled tensor: finite, and equal to the reference."""
    nH, H, group = 2, 128, 3
    lens = [1, 9, 40, 64]
    U = len(lens)
    g = torch.Generator().manual_seed(7)
    pad = torch.randn(U, 64, 2 * H, generator=g).to(BF)
    for u, L in enumerate(lens):
        pad[u, L:] = float("nan")
    KV = pad.view(U * 64, 2 * H).cuda()
    row0 = (torch.arange(U, dtype=torch.int32) * 64).cuda()
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    q = torch.randn(U * group, H, generator=g).to(BF).cuda()
    out = torch.zeros(U * group, H, dtype=BF, device="cuda")
    ops.decode_xattn(q, KV[:, :H], KV[:, H:], out, nH=nH, kv_row0=row0, kv_len=lens_d, Lkv_max=64, group=group)
    assert bool(torch.isfinite(out.float()).all())
    close(out, reference(q, KV[:, :H], KV[:, H:], row0.tolist(), lens, list(range(U)), group, nH), 2e-2, 2e-2, "padded, NaN behind the lengths")
    for last in (17, 16, 1):                                       # the last source ends the buffer: mid-block, on a block boundary, one row
        lens2 = [5, 33, last]
        KV2, row0_2, lens2_d = packed(lens2, [1, 0, 2], H, seed=8 + last, pad_rows=300, fill=float("nan"))
        assert int(row0_2[2]) + last == KV2.shape[0]
        q2 = torch.randn(3 * group, H, generator=g).to(BF).cuda()
        out2 = torch.zeros(3 * group, H, dtype=BF, device="cuda")
        ops.decode_xattn(q2, KV2[:, :H], KV2[:, H:], out2, nH=nH, kv_row0=row0_2, kv_len=lens2_d, Lkv_max=40, group=group)
        assert bool(torch.isfinite(out2.float()).all()), last
        close(out2, reference(q2, KV2[:, :H], KV2[:, H:], row0_2.tolist(), lens2, [0, 1, 2], group, nH), 2e-2, 2e-2, f"packed, buffer ends after {last}")
    # a length beyond Lkv_max read from memory is clamped to Lkv_max rows of the source (here: the whole source)
    big = torch.tensor([1000, 9, 40, 64], dtype=torch.int32).cuda()
    lens3 = [64, 9, 40, 64]
    pad3 = torch.randn(U, 64, 2 * H, generator=g).to(BF).cuda().view(U * 64, 2 * H)
    out3 = torch.zeros(U * group, H, dtype=BF, device="cuda")
    ops.decode_xattn(q, pad3[:, :H], pad3[:, H:], out3, nH=nH, kv_row0=row0, kv_len=big, Lkv_max=64, group=group)
    close(out3, reference(q, pad3[:, :H], pad3[:, H:], row0.tolist(), lens3, list(range(U)), group, nH), 2e-2, 2e-2, "clamped length")


def test_equal_lengths_are_the_existing_kernel_bit_for_bit(ops):
    """All sources 54 rows, 5 beams: the same bits as ops.decode_attn(..., kv_div=group) on the same buffers (one code path, the block count
    now per wave)."""
    nH, H, group, U, L = 2, 128, 5, 6, 54
    g = torch.Generator().manual_seed(9)
    KV = torch.randn(U * L, 2 * H, generator=g).to(BF).cuda()
    q = torch.randn(U * group, H, generator=g).to(BF).cuda()
    want = torch.zeros(U * group, H, dtype=BF, device="cuda")
    ops.decode_attn(q, KV[:, :H], KV[:, H:], want, nH=nH, Lkv=L, seq_stride=L * 2 * H, tok_stride=2 * H, kv_div=group, group=group)
    got = torch.zeros_like(want)
    ops.decode_xattn(q, KV[:, :H], KV[:, H:], got, nH=nH, kv_row0=(torch.arange(U, dtype=torch.int32) * L).cuda(),
                     kv_len=torch.full((U,), L, dtype=torch.int32).cuda(), Lkv_max=L, group=group)
    assert torch.equal(got, want)


def test_bad_arguments_are_refused(ops):
    q = torch.zeros(6, 128, dtype=BF, device="cuda")
    kv = torch.zeros(40, 256, dtype=BF, device="cuda")
    i32 = torch.ones(6, dtype=torch.int32, device="cuda")
    for kw in (dict(group=4), dict(Lkv_max=300), dict(Lkv_max=0)):
        args = dict(nH=2, kv_row0=i32, kv_len=i32, Lkv_max=16, group=2)
        args.update(kw)
        with pytest.raises(RuntimeError, match="spmm_decode_xattn"):
            ops.decode_xattn(q, kv[:, :128], kv[:, 128:], q.clone(), **args)


# ------------------------------------------------------------------------------------------------------------------ beam step
def _logits(R, V, g, sep_id):
    logits = torch.randn(R, V, generator=g) * 2.0
    boost = torch.rand(R, generator=g) < 0.3
    logits[:, sep_id] += torch.where(boost, torch.full((R,), 6.0), torch.full((R,), -2.0))
    return logits.cuda()


def _same_state(fus, ref, sel=None, tag=""):
    F = ref.F
    pick = (lambda x: x) if sel is None else (lambda x: x[sel])
    assert torch.equal(pick(fus.done), ref.done) and torch.equal(pick(fus.fin_n).long(), ref.fin_n), tag
    assert torch.equal(pick(fus.tokens).long(), ref.tokens), tag
    torch.testing.assert_close(pick(fus.cur_p), ref.cur_p, rtol=0, atol=2e-5)
    fp_f, fp_r = pick(fus.fin_p)[:, :F], ref.fin_p[:, :F]
    assert torch.equal(torch.isinf(fp_f), torch.isinf(fp_r)), tag
    torch.testing.assert_close(torch.where(torch.isinf(fp_f), torch.zeros_like(fp_f), fp_f), torch.where(torch.isinf(fp_r), torch.zeros_like(fp_r), fp_r),
                               rtol=0, atol=2e-5)
    used = torch.arange(F, device="cuda")[None, :] < ref.fin_n[:, None]
    assert torch.equal(pick(fus.fin_len)[:, :F].long()[used], ref.fin_len[:, :F][used]), tag
    assert torch.equal(pick(fus.fin_tok)[:, :F].long()[used], ref.fin_tok[:, :F][used]), tag


@pytest.mark.parametrize("N,k,V", [(3, 1, 16), (4, 2, 20), (6, 5, 300), (2, 8, 64)])
def test_beam_step_until_matches_tensor_bookkeeping(N, k, V):
    """spmm_beam_step_until with need = k*k against BeamBook(need=k*k).update + the ancestry reorder, position by position for 10 positions:
    finals in the same slots, survivors, histories, scores, ancestry, tokens to feed; F = k*k + k slots are never exceeded."""
    from spmm_amd import decode
    T, need = 10, k * k
    L, R = T + 3, N * k
    g = torch.Generator().manual_seed(3 + N)
    ref, fus = decode.BeamBook(N, k, T, "cuda", need=need), decode.BeamBook(N, k, T, "cuda", fused=True, need=need)
    v0 = torch.randn(N, k, generator=g).cuda()
    i0 = torch.stack([torch.randperm(V - 4, generator=g)[:k] + 4 for _ in range(N)]).cuda()
    ref.first(v0, i0)
    fus.first(v0, i0)
    rows = torch.arange(R, dtype=torch.int32, device="cuda")
    anc_ref = rows[:, None].repeat(1, L).contiguous()
    anc_fus = anc_ref.clone()
    for s in range(T):
        logits = _logits(R, V, g, decode.SEP_ID)
        values, indices = decode._pick(torch.softmax(logits.view(N, k, -1), dim=-1), k, False)
        parent, tok = ref.update(values, indices)
        anc_ref = anc_ref.view(N, k, L).gather(1, parent[:, :, None].expand(N, k, L).long()).reshape(R, L).contiguous()
        anc_ref[:, s + 2:] = rows[:, None]
        ids = fus.step_fused(logits, anc_fus)
        _same_state(fus, ref, tag=f"position {s}")
        assert int(fus.n_done) == int(ref.done.sum()) and int(fus.fin_n.max()) <= fus.F
        lr = (~ref.done)[:, None].expand(N, k).reshape(R)
        assert torch.equal(ids.long()[lr], tok.reshape(R)[lr]) and torch.equal(anc_fus[lr], anc_ref[lr]), s
        anc_ref = torch.where(lr[:, None], anc_ref, anc_fus)
    assert int(ref.fin_n.max()) > k or k == 1                      # the search went on past k finals
    got, want = fus.results(), ref.results()
    assert [[h[1] for h in m] for m in got] == [[h[1] for h in m] for m in want]


def test_beam_step_until_on_a_compacted_batch():
    """After a compaction the kernel sees the live molecules only (`mol`: their state index, `rowmap`: the cache rows of their beams): the
    kept molecules advance exactly as the tensor-op book of those molecules alone, the others' state is not touched, and "the row itself"
    in the ancestry table is the row map's entry."""
    from spmm_amd import decode
    N, k, V, T = 6, 3, 40, 10
    need, L = k * k, T + 3
    g = torch.Generator().manual_seed(17)
    fus = decode.BeamBook(N, k, T, "cuda", fused=True, need=need)
    v0 = torch.randn(N, k, generator=g).cuda()
    i0 = torch.stack([torch.randperm(V - 4, generator=g)[:k] + 4 for _ in range(N)]).cuda()
    fus.first(v0, i0)
    anc = torch.arange(N * k, dtype=torch.int32, device="cuda")[:, None].repeat(1, L).contiguous()
    for s in range(2):
        fus.step_fused(_logits(N * k, V, g, decode.SEP_ID), anc)
    keep = torch.tensor([1, 2, 4], device="cuda")
    n = keep.numel()
    ref = decode.BeamBook(n, k, T, "cuda", need=need)              # the tensor-op book of the kept molecules alone, from the same state
    ref.tokens, ref.cur_p, ref.t = fus.tokens[keep].long().clone(), fus.cur_p[keep].clone(), fus.t
    ref.fin_p, ref.fin_len, ref.fin_tok = fus.fin_p[keep].clone(), fus.fin_len[keep].long().clone(), fus.fin_tok[keep].long().clone()
    ref.fin_n, ref.done = fus.fin_n[keep].long().clone(), fus.done[keep].clone()
    before = {nm: getattr(fus, nm).clone() for nm in ("tokens", "cur_p", "fin_p", "fin_len", "fin_tok", "fin_n", "done")}
    fus.compact(keep)
    rowmap = (torch.arange(N * k, dtype=torch.int32, device="cuda").view(N, k)[keep].reshape(-1) + 100).contiguous()
    anc_c = anc.view(N, k, L)[keep].reshape(n * k, L).contiguous()
    anc_ref = anc_c.clone()
    for s in range(2, T):
        logits = _logits(n * k, V, g, decode.SEP_ID)
        values, indices = decode._pick(torch.softmax(logits.view(n, k, -1), dim=-1), k, False)
        parent, tok = ref.update(values, indices)
        anc_ref = anc_ref.view(n, k, L).gather(1, parent[:, :, None].expand(n, k, L).long()).reshape(n * k, L).contiguous()
        anc_ref[:, s + 2:] = rowmap[:, None]
        ids = fus.step_fused(logits, anc_c, rowmap=rowmap)
        _same_state(fus, ref, sel=keep, tag=f"position {s}")
        lr = (~ref.done)[:, None].expand(n, k).reshape(n * k)
        assert torch.equal(ids.long()[lr], tok.reshape(n * k)[lr]) and torch.equal(anc_c[lr], anc_ref[lr]), s
        anc_ref = torch.where(lr[:, None], anc_ref, anc_c)
    gone = torch.tensor([0, 3, 5], device="cuda")
    for nm, t in before.items():
        assert torch.equal(getattr(fus, nm)[gone], t[gone]), nm


@pytest.mark.parametrize("N,k,V", [(4, 2, 20), (6, 5, 300)])
def test_need_k_through_the_new_entry_is_spmm_beam_step(N, k, V):
    """need = k through spmm_beam_step_until leaves, bit for bit, the state spmm_beam_step leaves."""
    from spmm_amd import decode, ops
    T, L, R = 10, 13, N * k
    g = torch.Generator().manual_seed(5)
    a, b = decode.BeamBook(N, k, T, "cuda", fused=True), decode.BeamBook(N, k, T, "cuda", fused=True)
    v0 = torch.randn(N, k, generator=g).cuda()
    i0 = torch.stack([torch.randperm(V - 4, generator=g)[:k] + 4 for _ in range(N)]).cuda()
    a.first(v0, i0)
    b.first(v0, i0)
    anc_a = torch.arange(R, dtype=torch.int32, device="cuda")[:, None].repeat(1, L).contiguous()
    anc_b = anc_a.clone()
    for s in range(T):
        logits = _logits(R, V, g, decode.SEP_ID)
        ia = ops.beam_step(logits, a, t=a.t, anc=anc_a)
        ib = ops.beam_step(logits, b, t=b.t, anc=anc_b, need=k)
        a.t += 1
        b.t += 1
        assert torch.equal(ia, ib) and torch.equal(anc_a, anc_b)
        for nm in ("tokens", "cur_p", "fin_p", "fin_len", "fin_tok", "fin_n", "done", "n_done"):
            assert torch.equal(getattr(a, nm), getattr(b, nm)), (s, nm)
    assert bool(a.done.any())
