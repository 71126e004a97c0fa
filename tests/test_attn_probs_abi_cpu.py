"""spmm_attn_probs' argument checks (csrc/attnmap.hip), exercised where there is no GPU: every call below is one the entry point refuses
BEFORE a launch -- never add a case here that is complete (this file also runs where there is a GPU)."""
import ctypes
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


def _args(Q=P_, ldq=128, K=P_, ldk=256, kmask=None, kv_seq=None, q_row0=None, q_len=None, kv_row0=None, kv_len=None, P_mean=P_, P_heads=P_,
          ldp=56, head_stride=56 * 40, nseq=2, nH=2, Lq=20, Lkv=54):
    return (Q, ldq, K, ldk, kmask, kv_seq, q_row0, q_len, kv_row0, kv_len, P_mean, P_heads, ldp, head_stride, nseq, nH, Lq, Lkv, None)


MIS16 = r"misaligned Q / K \(16 bytes\)"
MIS4 = r"misaligned P_mean / P_heads / kmask / kv_seq / q_row0 / q_len / kv_row0 / kv_len \(4 bytes\)"
PAIRS = "q_row0/q_len and kv_row0/kv_len must be given in pairs"
REFUSED = [
    (_args(Q=None), "Q and K are required"),
    (_args(K=None), "Q and K are required"),
    (_args(P_mean=None, P_heads=None), "P_mean or P_heads is required"),
    (_args(Q=P_ + 8), MIS16),
    (_args(K=P_ + 2), MIS16),
    (_args(P_mean=P_ + 2), MIS4),
    (_args(P_heads=P_ + 1), MIS4),
    (_args(kmask=P_ + 3), MIS4),
    (_args(kv_seq=P_ + 2), MIS4),
    (_args(q_row0=P_ + 1, q_len=P_), MIS4),
    (_args(q_row0=P_, q_len=P_ + 2), MIS4),
    (_args(kv_row0=P_ + 2, kv_len=P_), MIS4),
    (_args(kv_row0=P_, kv_len=P_ + 1), MIS4),
    (_args(nH=0), r"nH=0 \(1 <= nH <= 16\)"),
    (_args(nH=17, ldq=2048, ldk=2048), r"nH=17 \(1 <= nH <= 16\)"),
    (_args(ldq=127), r"ldq=127 ldk=256 must be >= nH\*64=128"),
    (_args(ldk=64), r"ldq=128 ldk=64 must be >= nH\*64=128"),
    (_args(ldq=132), "ldq=132 ldk=256 must be multiples of 8"),
    (_args(Lq=0), r"Lq=0 Lkv=54 \(1 <= Lq, Lkv <= 256\)"),
    (_args(Lq=257), "Lq=257 Lkv=54"),
    (_args(Lkv=0), "Lq=20 Lkv=0"),
    (_args(Lkv=257, ldp=300, head_stride=30000), "Lq=20 Lkv=257"),
    (_args(ldp=53), "ldp=53 must be >= Lkv=54"),
    (_args(nseq=-1), r"nseq=-1 \(nseq >= 0\)"),
    (_args(q_row0=P_), PAIRS),
    (_args(q_len=P_), PAIRS),
    (_args(kv_row0=P_), PAIRS),
    (_args(kv_len=P_), PAIRS),
    (_args(head_stride=0), "head_stride=0 must be positive and >= ldp=56"),
    (_args(head_stride=-5), "head_stride=-5 must be positive"),
    (_args(head_stride=55), "head_stride=55 must be positive and >= ldp=56"),
    (_args(nseq=0, nH=0), "nH=0"),                                 # nseq == 0 skips the launch, not the checks of the arguments
    (_args(nseq=0, P_mean=None, P_heads=None), "P_mean or P_heads is required"),
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[1][:24].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_attn_probs_refuses_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument, with spmm_last_error set; "launch failed" (rc = 2) on a machine
    without a GPU would mean the call got as far as the launch."""
    from spmm_amd._lib import lib
    args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_attn_probs", *args)
    assert "spmm_attn_probs failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert "spmm_attn_probs:" in str(e.value)
    assert lib().cdll.spmm_last_error().decode() in str(e.value)


def test_no_sequences_is_no_launch(built):
    """nseq == 0 returns 0 before anything is dereferenced or launched: no GPU needed.  One head needs no head stride."""
    from spmm_amd._lib import lib
    lib().call("spmm_attn_probs", *_args(nseq=0))
    lib().call("spmm_attn_probs", *_args(nseq=0, P_mean=None))
    lib().call("spmm_attn_probs", *_args(nseq=0, P_heads=None, head_stride=0))
    lib().call("spmm_attn_probs", *_args(nseq=0, nH=1, ldq=64, ldk=64, head_stride=0))
    lib().call("spmm_attn_probs", *_args(nseq=0, q_row0=P_, q_len=P_, kv_row0=P_, kv_len=P_, kv_seq=P_, kmask=P_))


def test_the_header_declares_and_the_library_exports_the_entry_point(built):
    from spmm_amd._lib import lib, parse_header
    res, argtypes = parse_header()["spmm_attn_probs"]
    i, l, p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert res is ctypes.c_int and argtypes == [p, l, p, l, p, p, p, p, p, p, p, p, l, l, i, i, i, i, p]
    assert hasattr(lib().cdll, "spmm_attn_probs")
    with open(os.path.join(ROOT, "include", "spmm_hip.h")) as f:
        src = f.read()
    assert "int spmm_attn_probs(const void* Q, long ldq, const void* K, long ldk, const int* kmask, const int* kv_seq," in src
    assert "xbert.py:305-340" in src


def test_the_wrapper_passes_the_header_s_prototype():
    """ops.attn_probs in dry-run mode: the argument list matches the header; column blocks of fused buffers and given outputs pass."""
    import torch
    from spmm_amd import ops
    Q, KV = torch.zeros(40, 384, dtype=torch.bfloat16), torch.zeros(108, 256, dtype=torch.bfloat16)
    i32 = torch.zeros(2, dtype=torch.int32)
    ops._DRY_RUN, ops._dry_log[:] = True, []
    try:
        pm, ph = ops.attn_probs(Q[:, :128], KV[:, :128], nseq=2, nH=2, Lq=20, Lkv=54)
        assert tuple(pm.shape) == (40, 54) and pm.dtype == torch.float32 and ph is None
        pm, ph = ops.attn_probs(Q[:, 128:256], KV[:, :128], nseq=2, nH=2, Lq=20, Lkv=54, mean=False, heads=True, kv_seq=i32, q_row0=i32, q_len=i32,
                                kv_row0=i32, kv_len=i32)
        assert pm is None and tuple(ph.shape) == (2, 40, 54)
        out = torch.zeros(40, 60)
        assert ops.attn_probs(Q[:, :128], KV[:, :128], nseq=2, nH=2, Lq=20, Lkv=54, P_mean=out)[0] is out
        with pytest.raises(AssertionError):
            ops.attn_probs(Q[:, :128].float(), KV[:, :128], nseq=2, nH=2, Lq=20, Lkv=54)
        with pytest.raises(AssertionError):
            ops.attn_probs(Q[:, :128], KV[:, :128], nseq=2, nH=2, Lq=20, Lkv=54, mean=False)
    finally:
        ops._DRY_RUN = False
    assert ops._dry_log == ["spmm_attn_probs"] * 3
