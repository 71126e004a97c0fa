"""spmm_sim_topk (csrc/retrieve.hip) against float64 on the CPU.  Features are random unit vectors.

Tolerance.  A returned score must lie within 2 E 2^-24 of the float64 dot product at the returned index: the fp32 accumulation bound of a
sum of E products of unit vectors (|sum| <= 1, E roundings of the products and E of the partial sums, each at most 2^-24 relative to a
magnitude <= 1): 3.1e-5 at E = 256, 7.6e-6 at E = 64, 6.1e-5 at E = 512.  The j-th returned score must be at least the true j-th largest minus the same bound,
which is robust to near ties without demanding identical indices.  No index is repeated and every index lies in [base, base + N)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


def _unit(rows, E, seed):
    x = torch.randn(rows, E, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float()


def _state(Q, k):
    return (torch.full((Q, k), 7.0, dtype=torch.float32, device="cuda"), torch.full((Q, k), 12345, dtype=torch.int64, device="cuda"))


def _run(q, f, k, base=0, chunks=None, state=None, cut=None):
    """-> (scores, index) on the CPU.  chunks: row counts of the pieces the library is streamed in (None: one call)."""
    from spmm_amd import ops
    scores, index = _state(q.shape[0], k) if state is None else state
    N = f.shape[0]
    chunks = [N] if chunks is None else chunks
    assert sum(chunks) == N
    r0 = 0
    for i, n in enumerate(chunks):
        ops.sim_topk(q, f[r0:r0 + n], scores, index, base=base + r0, merge=(i > 0 or state is not None), cut=cut)
        r0 += n
    torch.cuda.synchronize()
    return scores.cpu(), index.cpu()


def _check(scores, index, S64, base, k, E, first_rank=0):
    """The contract of the docstring for the ranks first_rank .. first_rank + k - 1 of every query."""
    Q, N = S64.shape
    tol = 2 * E * 2.0 ** -24
    m = max(0, min(N - first_rank, k))
    true = S64.sort(dim=1, descending=True).values[:, first_rank:first_rank + m]
    idx = index[:, :m] - base
    assert bool(((idx >= 0) & (idx < N)).all()), "an index outside [base, base + N)"
    for j in range(Q):
        assert idx[j].unique().numel() == m, f"query {j}: a repeated index"
    at = S64.gather(1, idx)
    err = (scores[:, :m].double() - at).abs().max().item() if m else 0.0
    short = (true - scores[:, :m].double()).max().item() if m else 0.0
    print(f"[sim_topk] Q={Q} N={N} k={k} E={E}: max |score - f64 at index| {err:.3e}, max (true j-th - returned j-th) {short:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, tol)
    assert short <= tol, (short, tol)
    if m > 1:
        assert bool((scores[:, 1:m] <= scores[:, :m - 1]).all()), "scores not in descending order"
    assert bool((scores[:, m:] == NEG_INF).all()) and bool((index[:, m:] == -1).all()), "tail slots are not (-inf, -1)"


CASES = [  # (E, Q, N, k): every value of every axis, tails of the 16-query and 256-row tiles, N < k, more than one workgroup per query tile
    (64, 1, 1, 1), (64, 1, 63, 64), (64, 17, 64, 5), (64, 65, 65, 64), (64, 1, 1000, 5), (64, 17, 4097, 64), (64, 65, 1000, 1), (64, 17, 1, 5),
    (256, 1, 1, 64), (256, 17, 63, 5), (256, 65, 64, 1), (256, 1, 65, 64), (256, 65, 1000, 64), (256, 1, 4097, 5), (256, 17, 4097, 1),
    (256, 65, 4097, 5), (256, 17, 65, 64), (256, 1, 64, 5), (64, 65, 63, 64), (256, 17, 1000, 64),
    (512, 17, 1000, 64),      # the widest feature the entry point takes: the largest LDS footprint (49 664 bytes), eight 64-element trips
]


@pytest.mark.parametrize("E,Q,N,k", CASES, ids=[f"E{e}-Q{q}-N{n}-k{k}" for e, q, n, k in CASES])
def test_topk_matches_float64(E, Q, N, k):
    q, f = _unit(Q, E, 1), _unit(N, E, 2)
    S64 = q.double() @ f.double().T
    scores, index = _run(q.cuda(), f.cuda(), k)
    _check(scores, index, S64, 0, k, E)


@pytest.fixture(scope="module")
def lib4097():
    E, Q, N = 256, 17, 4097
    q, f = _unit(Q, E, 11), _unit(N, E, 12)
    return q, f, q.double() @ f.double().T


def test_chunked_streaming_is_bit_identical(lib4097):
    """N = 4097 in one call, as chunks of 1000 and as chunks of 1, 64, 4032: bit-identical scores, equal indices."""
    q, f, S64 = lib4097
    qd, fd = q.cuda(), f.cuda()
    for k in (5, 64):
        one = _run(qd, fd, k)
        _check(*one, S64, 0, k, 256)
        for chunks in ([1000, 1000, 1000, 1000, 97], [1, 64, 4032]):
            got = _run(qd, fd, k, chunks=chunks)
            assert torch.equal(got[0].view(torch.int32), one[0].view(torch.int32)), (k, chunks)
            assert torch.equal(got[1], one[1]), (k, chunks)


def test_ties_come_back_adjacent_in_ascending_index(lib4097):
    """Rows 3, 300 and 3000 are copies of one vector: equal scores bit for bit, adjacent, ascending index -- for the query that is that
    vector (ranks 0..2) and for every other query in whose list they appear."""
    q, f, _ = lib4097
    f = f.clone()
    f[300] = f[3]
    f[3000] = f[3]
    q = q.clone()
    q[0] = f[3]
    S64 = q.double() @ f.double().T
    for chunks in (None, [5, 295, 2700, 1097]):
        scores, index = _run(q.cuda(), f.cuda(), 64, chunks=chunks)
        _check(scores, index, S64, 0, 64, 256)
        assert index[0, :3].tolist() == [3, 300, 3000], index[0, :5].tolist()
        assert abs(scores[0, 0].item() - 1.0) <= 2 * 256 * 2.0 ** -24
        for j in range(q.shape[0]):
            row = index[j].tolist()
            hit = [p for p, i in enumerate(row) if i in (3, 300, 3000)]
            if len(hit) == 3:
                assert hit == [hit[0], hit[0] + 1, hit[0] + 2] and [row[p] for p in hit] == [3, 300, 3000], (j, row)
                assert scores[j, hit[0]] == scores[j, hit[1]] == scores[j, hit[2]]
            elif hit:                                    # the list ends inside the run of equal candidates: it keeps the run's head
                assert hit == list(range(64 - len(hit), 64)) and [row[p] for p in hit] == [3, 300, 3000][:len(hit)], (j, row)


def test_base_beyond_int32(lib4097):
    q, f, S64 = lib4097
    for base in (2 ** 31 + 5, 2 ** 40 + 123):
        scores, index = _run(q.cuda(), f.cuda(), 5, base=base, chunks=[1000, 3097])
        _check(scores, index, S64, base, 5, 256)
        ref = _run(q.cuda(), f.cuda(), 5)
        assert torch.equal(index - base, ref[1]) and torch.equal(scores, ref[0])


def test_zero_rows(lib4097):
    from spmm_amd import ops
    q, f, _ = lib4097
    qd, fd = q.cuda(), f.cuda()
    scores, index = _run(qd, fd, 5)
    st = (scores.cuda(), index.cuda())
    ops.sim_topk(qd, fd[:0], st[0], st[1], base=77, merge=True)              # n = 0, merge = 1: a no-op
    torch.cuda.synchronize()
    assert torch.equal(st[0].cpu(), scores) and torch.equal(st[1].cpu(), index)
    ops.sim_topk(qd, fd[:0], st[0], st[1], merge=False)                      # n = 0, merge = 0: nothing seen
    torch.cuda.synchronize()
    assert bool((st[0].cpu() == NEG_INF).all()) and bool((st[1].cpu() == -1).all())


def test_row_strides(lib4097):
    """q and f as column slices of wider matrices (row strides E + 8 and E + 12, a 16-byte aligned first element)."""
    q, f, _ = lib4097
    qw = torch.randn(q.shape[0], 256 + 8).cuda()
    fw = torch.randn(f.shape[0], 256 + 12).cuda()
    qw[:, :256] = q.cuda()
    fw[:, 4:260] = f.cuda()
    got = _run(qw[:, :256], fw[:, 4:260], 64)
    ref = _run(q.cuda(), f.cuda(), 64)
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1])


def test_nan_row_ranks_below_every_number():
    E, Q = 64, 17
    q, f = _unit(Q, E, 21), _unit(1000, E, 22)
    f[7] = float("nan")
    S64 = q.double() @ f.double().T
    S64[:, 7] = NEG_INF
    scores, index = _run(q.cuda(), f.cuda(), 64, chunks=[5, 995])
    assert not bool((index == 7).any()) and bool(torch.isfinite(scores).all())
    _check(scores, index, S64, 0, 64, E)
    # fewer numbers than k: the NaN row comes after every number and before the empty slots
    scores, index = _run(q.cuda(), f[5:10].cuda(), 8, base=5)
    assert bool((index[:, 4] == 7).all()) and bool(torch.isnan(scores[:, 4]).all())
    assert bool((index[:, 5:] == -1).all()) and bool((scores[:, 5:] == NEG_INF).all())
    assert bool(torch.isfinite(scores[:, :4]).all()) and sorted(index[0, :4].tolist()) == [5, 6, 8, 9]


def test_two_launches_are_bit_identical(lib4097):
    q, f, _ = lib4097
    a = _run(q.cuda(), f.cuda(), 64)
    b = _run(q.cuda(), f.cuda(), 64)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_cut_continues_a_ranking_past_64(lib4097):
    """Ranks 64..127 from a second pass whose cut is the first pass's last entry: together the 128 best, nothing twice."""
    q, f, S64 = lib4097
    qd, fd = q.cuda(), f.cuda()
    s1, i1 = _run(qd, fd, 64)
    cut = (s1[:, 63].contiguous().cuda(), i1[:, 63].contiguous().cuda())
    s2, i2 = _run(qd, fd, 64, chunks=[2000, 2097], cut=cut)
    _check(s2, i2, S64, 0, 64, 256, first_rank=64)
    both = torch.cat([i1, i2], 1)
    assert all(both[j].unique().numel() == 128 for j in range(both.shape[0]))
    assert bool((s2[:, 0] <= s1[:, 63]).all())
