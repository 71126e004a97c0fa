"""spmm_kv_prefill (csrc/prefill.hip) against a torch indexing reference.  The data AND the caches' initial contents are random 16-bit
patterns (NaN payloads, -0, denormals included), so a pure move is visible as such; each cache is an interior view of a larger buffer with
4 096 guard elements on each side, and the WHOLE buffer must equal the reference's: guards and untouched cells included."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096


def _bits(shape, gen):
    return torch.randint(-32768, 32768, shape, generator=gen, dtype=torch.int32).to(torch.int16)


def _run(nH, Lmax, R, row0, length, dst, src_rows, ld_mult, seed=0):
    """One launch on fresh buffers -> (got K buffer, got V buffer, want K buffer, want V buffer), int16 views on the host."""
    from spmm_amd import ops
    g = torch.Generator().manual_seed(seed)
    H = nH * 64
    ld = ld_mult * H
    src = _bits((src_rows, ld), g)                              # the [M, 3H] (or [M, 2H]) projection output; K | V = its last two column blocks
    kcol, vcol = ld - 2 * H, ld - H
    n_cache = R * nH * Lmax * 64
    bufs = [_bits((n_cache + 2 * GUARD,), g) for _ in range(2)]
    want = [b.clone() for b in bufs]
    for w, col in zip(want, (kcol, vcol)):
        cache = w[GUARD:GUARD + n_cache].view(R, nH, Lmax, 64)
        for r0, ln, d in zip(row0, length, dst):
            if not 0 <= d < R:
                continue
            for j in range(min(ln, Lmax)):
                if 0 <= r0 + j < src_rows:
                    cache[d, :, j, :] = src[r0 + j, col:col + H].view(nH, 64)
    src_d = src.cuda().view(torch.bfloat16)
    dev = [b.cuda() for b in bufs]
    Kc, Vc = (b[GUARD:GUARD + n_cache].view(torch.bfloat16).view(R, nH, Lmax, 64) for b in dev)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")                    # noqa: E731
    ops.kv_prefill(src_d[:, kcol:kcol + H], src_d[:, vcol:vcol + H], i32(row0), i32(length), i32(dst), Kc, Vc)
    torch.cuda.synchronize()
    return dev[0].cpu(), dev[1].cpu(), want[0], want[1]


CASES = {
    "one-token": dict(nH=2, Lmax=16, R=1, row0=[0], length=[1], dst=[0], src_rows=4, ld_mult=3),
    "three-entries-3H": dict(nH=2, Lmax=20, R=6, row0=[23, 0, 5], length=[20, 3, 17], dst=[4, 0, 2], src_rows=43, ld_mult=3),
    "three-entries-2H": dict(nH=2, Lmax=20, R=6, row0=[23, 0, 5], length=[20, 3, 17], dst=[4, 0, 2], src_rows=43, ld_mult=2),
    "published-heads-longest-cache": dict(nH=12, Lmax=256, R=3, row0=[131, 0, 1], length=[256, 1, 130], dst=[2, 0, 1], src_rows=387, ld_mult=3),
    "length-past-cache-and-source": dict(nH=2, Lmax=256, R=2, row0=[10], length=[300], dst=[1], src_rows=260, ld_mult=3),
    "empty-entry": dict(nH=2, Lmax=16, R=3, row0=[0, 2], length=[0, 5], dst=[0, 2], src_rows=9, ld_mult=3),
    "negative-length-and-row": dict(nH=2, Lmax=16, R=3, row0=[0, -2], length=[-3, 5], dst=[0, 2], src_rows=9, ld_mult=3),
    "destination-out-of-range": dict(nH=2, Lmax=16, R=3, row0=[0, 4, 8], length=[4, 4, 4], dst=[-1, 3, 1], src_rows=12, ld_mult=3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kv_prefill_is_an_exact_move_into_the_named_cells_only(name):
    c = CASES[name]
    gk, gv, wk, wv = _run(**c)
    assert torch.equal(gk, wk), f"{name}: keys differ in {(gk != wk).sum().item()} elements"
    assert torch.equal(gv, wv), f"{name}: values differ in {(gv != wv).sum().item()} elements"
    if name == "length-past-cache-and-source":               # exactly the positions j < 250 of row 1 were written
        n = 2 * 2 * 256 * 64
        before = _bits_before(c)
        changed = (gk[GUARD:GUARD + n] != before[GUARD:GUARD + n]).view(2, 2, 256, 64)
        assert not changed[0].any() and not changed[1, :, 250:].any() and changed[1, :, :250].any(dim=-1).all()
    if name == "destination-out-of-range":                   # only the last entry lands
        n = 3 * 2 * 16 * 64
        changed = (gk[GUARD:GUARD + n] != _bits_before(c)[GUARD:GUARD + n]).view(3, 2, 16, 64)
        assert not changed[0].any() and not changed[2].any() and changed[1, :, :4].any(dim=-1).all() and not changed[1, :, 4:].any()


def _bits_before(c):
    """The key buffer's initial contents of `_run(**c)` (same generator order)."""
    g = torch.Generator().manual_seed(0)
    H = c["nH"] * 64
    _bits((c["src_rows"], c["ld_mult"] * H), g)
    return _bits((c["R"] * c["nH"] * c["Lmax"] * 64 + 2 * GUARD,), g)


def test_no_entries_touch_nothing():
    from spmm_amd import ops
    g = torch.Generator().manual_seed(1)
    src = _bits((4, 384), g).cuda().view(torch.bfloat16)
    buf = _bits((2 * 2 * 16 * 64 + 2 * GUARD,), g)
    dev = buf.cuda()
    Kc = dev[GUARD:-GUARD].view(torch.bfloat16).view(2, 2, 16, 64)
    e = torch.empty(0, dtype=torch.int32, device="cuda")
    assert ops.kv_prefill(src[:, 128:256], src[:, 256:], e, e, e, Kc, Kc.clone()) is None
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), buf)
