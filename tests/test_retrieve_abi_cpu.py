"""spmm_sim_topk's argument checks (csrc/retrieve.hip), exercised where there is no GPU: every call below is one the entry point refuses
BEFORE a launch -- never add a case here that is complete (this file also runs where there is a GPU)."""
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


def _args(q=P_, ldq=256, f=P_, ldf=256, base=0, Q=4, n=100, E=256, k=8, scores=P_, index=P_, merge=0, cut_s=None, cut_i=None, ws=P_, ws_bytes=1 << 20):
    return (q, ldq, f, ldf, base, Q, n, E, k, scores, index, merge, cut_s, cut_i, ws, ws_bytes, None)


REFUSED = [
    (_args(k=0), r"k=0 must be in \[1,64\]"),
    (_args(k=65), r"k=65 must be in \[1,64\]"),
    (_args(E=96), "E=96 must be a multiple of 64 up to 512"),
    (_args(E=576), "E=576 must be a multiple of 64 up to 512"),
    (_args(E=0), "E=0 must be a multiple of 64 up to 512"),
    (_args(Q=0), "Q=0 must be at least 1"),
    (_args(n=-1), "n=-1 must be in"),
    (_args(n=2 ** 31), "must be in"),
    (_args(n=2 ** 31 - 255), r"must be in \[0, 2\^31 - 256\]"),
    (_args(merge=2), "merge=2 must be 0 or 1"),
    (_args(q=P_ + 4), "q / f must be 16-byte aligned"),
    (_args(f=P_ + 8), "q / f must be 16-byte aligned"),
    (_args(q=None), "null q / f"),
    (_args(f=None), "null q / f"),
    (_args(ldq=258), "ldq=258 ldf=256 must be multiples of 4"),
    (_args(ldf=255), "ldq=256 ldf=255 must be multiples of 4"),
    (_args(ldf=128), "ldq=256 ldf=128 must be multiples of 4, at least E=256"),
    (_args(scores=None), "null scores / index"),
    (_args(index=None), "null scores / index"),
    (_args(index=P_ + 4), "misaligned scores / index"),
    (_args(cut_s=P_), "cut_scores and cut_index come together"),
    (_args(cut_i=P_), "cut_scores and cut_index come together"),
    (_args(base=-1), "base=-1 out of range"),
    (_args(ws=None), "workspace of"),
    (_args(ws=P_ + 8), "workspace of"),
    (_args(ws_bytes=8), "workspace of 256 bytes"),
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[1][:24].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_sim_topk_refuses_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument; "launch failed" (rc = 2) on a machine without a GPU would mean
    the call got as far as the launch."""
    from spmm_amd._lib import lib
    args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_sim_topk", *args)
    assert "spmm_sim_topk failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert "spmm_sim_topk:" in str(e.value)


def test_workspace_query(built):
    """The workspace holds one 8-byte key per (row split, query, slot); a chunk of one 256-row tile has one split."""
    from spmm_amd._lib import lib
    L = lib().cdll
    assert L.spmm_sim_topk_workspace_bytes(4, 100, 8) == 4 * 8 * 8
    assert L.spmm_sim_topk_workspace_bytes(1, 0, 1) == 16
    big = L.spmm_sim_topk_workspace_bytes(64, 1_000_000, 64)
    assert big % 8 == 0 and 64 * 64 * 8 <= big <= 1 << 26
    assert L.spmm_sim_topk_workspace_bytes(0, 10, 1) == 0
