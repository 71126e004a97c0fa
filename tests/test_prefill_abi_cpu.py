"""spmm_kv_prefill's argument checks (csrc/prefill.hip), exercised where there is no GPU: every call below is one the entry point refuses
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


def _args(K=P_, V=P_, ld=384, src_rows=40, row0=P_, length=P_, dst_row=P_, E=3, Kc=P_, Vc=P_, R=6, nH=2, Lmax=20):
    return (K, V, ld, src_rows, row0, length, dst_row, E, Kc, Vc, R, nH, Lmax, None)


REQUIRED = "K, V, Kc, Vc, row0, len and dst_row are required"
ALIGNED = "K, V, Kc and Vc must be 16-byte aligned"
REFUSED = [
    (_args(K=None), REQUIRED),
    (_args(V=None), REQUIRED),
    (_args(Kc=None), REQUIRED),
    (_args(Vc=None), REQUIRED),
    (_args(row0=None), REQUIRED),
    (_args(length=None), REQUIRED),
    (_args(dst_row=None), REQUIRED),
    (_args(nH=0), r"nH=0 ld=384 \(nH >= 1, nH\*64 <= ld\)"),
    (_args(nH=-1), r"nH=-1 ld=384"),
    (_args(nH=7), r"nH=7 ld=384 \(nH >= 1, nH\*64 <= ld\)"),
    (_args(ld=132), "ld=132 must be a multiple of 8"),
    (_args(ld=388), "ld=388 must be a multiple of 8"),
    (_args(K=P_ + 8), ALIGNED),
    (_args(V=P_ + 2), ALIGNED),
    (_args(Kc=P_ + 4), ALIGNED),
    (_args(Vc=P_ + 8), ALIGNED),
    (_args(Lmax=0), r"Lmax=0 outside \[1, 256\]"),
    (_args(Lmax=257), r"Lmax=257 outside \[1, 256\]"),
    (_args(R=0), "E=3 R=0 src_rows=40"),
    (_args(E=-1), "E=-1 R=6 src_rows=40"),
    (_args(src_rows=0), "E=3 R=6 src_rows=0"),
    (_args(E=0, nH=0), "nH=0"),                      # E == 0 skips the launch, not the shape checks
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[1][:24].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_kv_prefill_refuses_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument, with spmm_last_error set; "launch failed" (rc = 2) on a machine
    without a GPU would mean the call got as far as the launch."""
    from spmm_amd._lib import lib
    args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_kv_prefill", *args)
    assert "spmm_kv_prefill failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert "spmm_kv_prefill:" in str(e.value)
    assert lib().cdll.spmm_last_error().decode() in str(e.value)


def test_no_entries_is_no_launch(built):
    """E == 0 returns 0 before anything is dereferenced or launched: null arrays, no GPU needed."""
    from spmm_amd._lib import lib
    lib().call("spmm_kv_prefill", *_args(K=None, V=None, row0=None, length=None, dst_row=None, Kc=None, Vc=None, E=0))


def test_the_header_declares_and_the_library_exports_the_entry_point(built):
    from spmm_amd._lib import lib, parse_header
    res, argtypes = parse_header()["spmm_kv_prefill"]
    assert res is ctypes.c_int and len(argtypes) == 14
    assert argtypes[:4] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long] and argtypes[7] is ctypes.c_int
    assert hasattr(lib().cdll, "spmm_kv_prefill")
    with open(os.path.join(ROOT, "include", "spmm_hip.h")) as f:
        assert "int spmm_kv_prefill(const void* K, const void* V, long ld, long src_rows" in f.read()
