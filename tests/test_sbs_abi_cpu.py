"""spmm_sbs_step's argument checks (csrc/sbs.hip), exercised where there is no GPU: every call below is one the entry point refuses BEFORE
a launch -- never add a case here that is complete (this file also runs where there is a GPU)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P_ = 0x1000       # "some non-null, aligned pointer": never dereferenced
NAMES = ("logits", "ldl", "noise", "ldn", "G", "W", "V", "Lmax", "t", "t_ptr", "t_off", "phi_in", "gum_in", "fin_in", "len_in", "tokens_in", "anc_in",
         "phi_out", "gum_out", "fin_out", "len_out", "tokens_out", "anc_out", "anc_ld", "ids_out", "parent_out", "open_out", "ws")
INS = ("phi_in", "gum_in", "fin_in", "len_in", "tokens_in", "anc_in")
OUTS = ("phi_out", "gum_out", "fin_out", "len_out", "tokens_out", "anc_out")


@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return so


def _args(**kw):
    a = dict(logits=P_, ldl=304, noise=P_ + 0x100, ldn=300, G=2, W=24, V=300, Lmax=43, t=5, t_ptr=None, t_off=0, anc_ld=43, ids_out=P_ + 0x200,
             parent_out=None, open_out=P_ + 0x300, ws=P_ + 0x400)
    a.update({n: P_ + 0x1000 * (i + 1) for i, n in enumerate(INS)})
    a.update({n: P_ + 0x1000 * (i + 11) for i, n in enumerate(OUTS)})
    a.update(kw)
    return tuple(a[n] for n in NAMES) + (None,)


REQ_IN = r"every state array \(phi, gum, fin, len, tokens, anc\) _in is required"
REQ_OUT = "every state array _out, ids_out and open_out are required"
MISALIGNED = r"misaligned pointer \(4 bytes: everything but fin_in / fin_out; ws: 8\)"
ALIAS = r"an _out array aliases its _in twin \(the step is not in place\)"
REFUSED = [
    (_args(G=-1), r"G=-1 \(G >= 0\)"),
    (_args(W=0), r"W=0 \(1 <= W <= 1024\)"),
    (_args(W=1025), r"W=1025 \(1 <= W <= 1024\)"),
    (_args(V=3), r"V=3 \(4 <= V <= 512\)"),
    (_args(V=513, ldl=600, ldn=600), r"V=513 \(4 <= V <= 512\)"),
    (_args(Lmax=1, t=0, anc_ld=1), r"Lmax=1 \(2 <= Lmax <= 256\)"),
    (_args(Lmax=257, anc_ld=257), r"Lmax=257 \(2 <= Lmax <= 256\)"),
    (_args(t=-1), r"t=-1 Lmax=43 \(0 <= t < Lmax - 1\)"),
    (_args(t=42), "t=42 Lmax=43"),
    (_args(t=43), "t=43 Lmax=43"),
    (_args(ldl=299), "ldl=299 ldn=300 must be >= V=300"),
    (_args(ldn=299), "ldl=304 ldn=299 must be >= V=300"),
    (_args(anc_ld=42), "anc_ld=42 < Lmax=43"),
    (_args(G=1 << 21, W=1024), r"G\*W=2147483648 rows"),
    (_args(logits=None), "logits, noise and ws are required"),
    (_args(noise=None), "logits, noise and ws are required"),
    (_args(ws=None), "logits, noise and ws are required"),
] + [(_args(**{n: None}), REQ_IN) for n in INS] + [(_args(**{n: None}), REQ_OUT) for n in OUTS + ("ids_out", "open_out")] + [
    (_args(**{n: P_ + 0x7002}), MISALIGNED) for n in ("logits", "noise", "t_ptr", "phi_in", "gum_in", "len_in", "tokens_in", "anc_in", "phi_out", "gum_out",
                                                      "len_out", "tokens_out", "anc_out", "ids_out", "parent_out", "open_out", "ws")
] + [(_args(ws=P_ + 0x404), MISALIGNED)] + [(_args(**{i: P_ + 0x9000, o: P_ + 0x9000}), ALIAS) for i, o in zip(INS, OUTS)] + [
    (_args(G=0, W=0), "W=0"),                                    # G == 0 skips the launch, not the checks of the arguments
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[1][:24].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_sbs_step_refuses_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument, with spmm_last_error set; "launch failed" (rc = 2) on a machine
    without a GPU would mean the call got as far as the launch."""
    from spmm_amd._lib import lib
    args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_sbs_step", *args)
    assert "spmm_sbs_step failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert "spmm_sbs_step:" in str(e.value)
    assert lib().cdll.spmm_last_error().decode() in str(e.value)


def test_no_groups_is_no_launch(built):
    """G == 0 returns 0 before anything is dereferenced or launched: null arrays, no GPU needed."""
    from spmm_amd._lib import lib
    lib().call("spmm_sbs_step", *_args(G=0))
    lib().call("spmm_sbs_step", *_args(G=0, logits=None, noise=None, ws=None, ids_out=None, open_out=None, **{n: None for n in INS + OUTS}))
    lib().call("spmm_sbs_step", *_args(G=0, t=99, t_ptr=P_))


def test_the_header_declares_and_the_library_exports_the_entry_point(built):
    from spmm_amd._lib import lib, parse_header
    res, argtypes = parse_header()["spmm_sbs_step"]
    i, l, p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert res is ctypes.c_int and argtypes == [p, l, p, l, i, i, i, i, i, p, i] + [p] * 12 + [i, p, p, p, p, p]
    assert len(argtypes) == len(NAMES) + 1 and hasattr(lib().cdll, "spmm_sbs_step")
    with open(os.path.join(ROOT, "spmm_amd", "csrc", "Makefile")) as f:
        assert "sbs.hip" in f.read()


def test_the_wrapper_passes_the_header_s_prototype():
    """ops.sbs_step in dry-run mode on a DistinctBook with the kernel's state types: the argument list matches the header; the tensor-op
    book (float64 / int64 state) is refused by the wrapper."""
    import torch
    from spmm_amd import decode, ops
    book = decode.DistinctBook(2, 8, 20, "cpu", fused=True)
    logits, noise = torch.zeros(16, 300), torch.zeros(16, 304)[:, :300]
    ops._DRY_RUN, ops._dry_log[:] = True, []
    try:
        ids = ops.sbs_step(logits, noise, book, t=1)
        assert ids.dtype == torch.int32 and ids.shape == (16,) and book.ws.numel() == 2 * 16 * 300
        with pytest.raises(AssertionError):
            ops.sbs_step(logits, noise, decode.DistinctBook(2, 8, 20, "cpu", fused=False), t=1)
        with pytest.raises(AssertionError):
            ops.sbs_step(logits[:8], noise, book, t=1)
    finally:
        ops._DRY_RUN = False
    assert ops._dry_log == ["spmm_sbs_step"]
