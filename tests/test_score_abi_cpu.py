"""spmm_lm_score's argument checks (csrc/score.hip), exercised where there is no GPU: every call below is one the entry point refuses BEFORE
a launch -- never add a case here that is complete (this file also runs where there is a GPU)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P_ = 0x1000       # "some non-null, 16-byte aligned pointer": never dereferenced


@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return so


def _args(y=P_, ldy=768, Wd=P_, ldw=768, bias=P_, ids=P_, row_of=None, rows=40, nseq=2, L=20, V=300, H=768, seq_row0=None, seq_len=None,
          tok_lp=P_, seq_lp=P_, seq_n=P_):
    return (y, ldy, Wd, ldw, bias, ids, row_of, rows, nseq, L, V, H, seq_row0, seq_len, tok_lp, seq_lp, seq_n, None)


REQUIRED = "y, Wd, bias, ids, tok_lp, seq_lp and seq_n are required"
REFUSED = [
    (_args(y=None), REQUIRED),
    (_args(Wd=None), REQUIRED),
    (_args(bias=None), REQUIRED),
    (_args(ids=None), REQUIRED),
    (_args(tok_lp=None), REQUIRED),
    (_args(seq_lp=None), REQUIRED),
    (_args(seq_n=None), REQUIRED),
    (_args(H=96, ldy=96, ldw=96), "H=96 must be a multiple of 64 up to 1024"),
    (_args(H=1088, ldy=1088, ldw=1088), "H=1088 must be a multiple of 64 up to 1024"),
    (_args(H=0), "H=0 must be a multiple of 64 up to 1024"),
    (_args(V=1), r"V=1 must be in \[2,512\]"),
    (_args(V=513), r"V=513 must be in \[2,512\]"),
    (_args(rows=0, row_of=P_, seq_row0=P_, seq_len=P_), "rows=0 nseq=2 L=20"),
    (_args(rows=41, row_of=P_, seq_row0=P_, seq_len=P_), "rows=41 nseq=2 L=20"),
    (_args(L=1, rows=2), "rows=2 nseq=2 L=1"),
    (_args(ldy=704), "ldy=704 ldw=768 must be multiples of 8, at least H=768"),
    (_args(ldw=760), "ldy=768 ldw=760 must be multiples of 8, at least H=768"),
    (_args(ldy=772), "ldy=772 ldw=768 must be multiples of 8"),
    (_args(y=P_ + 8), "y / Wd must be 16-byte aligned"),
    (_args(Wd=P_ + 2), "y / Wd must be 16-byte aligned"),
    (_args(bias=P_ + 2), "misaligned bias"),
    (_args(row_of=P_ + 4), "misaligned bias"),
    (_args(seq_row0=P_), "seq_row0 and seq_len come together"),
    (_args(seq_len=P_), "seq_row0 and seq_len come together"),
    (_args(rows=30), "dense sequences .* need rows=30 == nseq\\*L=40"),
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[1][:24].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_lm_score_refuses_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument, with spmm_last_error set; "launch failed" (rc = 2) on a machine
    without a GPU would mean the call got as far as the launch."""
    from spmm_amd._lib import lib
    args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_lm_score", *args)
    assert "spmm_lm_score failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert "spmm_lm_score:" in str(e.value)
    assert lib().cdll.spmm_last_error().decode() in str(e.value)


def test_the_header_declares_the_entry_point(built):
    from spmm_amd._lib import lib
    res, argtypes = lib().protos["spmm_lm_score"]
    assert len(argtypes) == 18
