"""spmm_logit_warp's argument checks (csrc/warp.hip), exercised where there is no GPU: every call below is one the entry point refuses
BEFORE a launch -- never add a case here that is complete (this file also runs where there is a GPU)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P_ = 0x1000       # "some non-null, aligned pointer": never dereferenced
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return so


def _args(lc=P_, lu=P_, ld=304, R=6, V=300, w=1.5, temperature=0.8, top_k=20, top_p=0.9, min_keep=2, out=P_, ldo=300):
    return (lc, lu, ld, R, V, w, temperature, top_k, top_p, min_keep, out, ldo, None)


REQUIRED = "lc and out are required"
REFUSED = [
    (_args(lc=None), REQUIRED),
    (_args(out=None), REQUIRED),
    (_args(lc=None, lu=None, out=None), REQUIRED),
    (_args(R=-1), r"R=-1 \(R >= 0\)"),
    (_args(temperature=0.0), "temperature=0 must be finite and > 0"),
    (_args(temperature=-0.5), "temperature=-0.5 must be finite and > 0"),
    (_args(temperature=INF), "temperature=inf must be finite and > 0"),
    (_args(temperature=NAN), "temperature=-?nan must be finite and > 0"),
    (_args(top_p=0.0), r"top_p=0 outside \(0, 1\]"),
    (_args(top_p=-0.1), r"top_p=-0.1 outside \(0, 1\]"),
    (_args(top_p=1.5), r"top_p=1.5 outside \(0, 1\]"),
    (_args(top_p=NAN), r"top_p=-?nan outside \(0, 1\]"),
    (_args(top_k=-1), "top_k=-1"),
    (_args(w=INF), "w=inf must be finite"),
    (_args(w=-INF), "w=-inf must be finite"),
    (_args(w=NAN), "w=-?nan must be finite"),
    (_args(min_keep=0), r"min_keep=0 V=300 \(1 <= min_keep <= 8, min_keep <= V <= 512\)"),
    (_args(min_keep=9), "min_keep=9 V=300"),
    (_args(V=513, ld=600, ldo=600), "min_keep=2 V=513"),
    (_args(V=1, min_keep=2), "min_keep=2 V=1"),
    (_args(V=0), "min_keep=2 V=0"),
    (_args(ld=299), "ld=299 ldo=300 must be >= V=300"),
    (_args(ldo=299), "ld=304 ldo=299 must be >= V=300"),
    (_args(lc=P_ + 2), r"misaligned lc / lu / out \(4 bytes\)"),
    (_args(lu=P_ + 1), r"misaligned lc / lu / out \(4 bytes\)"),
    (_args(R=0, temperature=0.0), "temperature=0"),              # R == 0 skips the launch, not the checks of the arguments
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[1][:24].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_logit_warp_refuses_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument, with spmm_last_error set; "launch failed" (rc = 2) on a machine
    without a GPU would mean the call got as far as the launch."""
    from spmm_amd._lib import lib
    args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_logit_warp", *args)
    assert "spmm_logit_warp failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert "spmm_logit_warp:" in str(e.value)
    assert lib().cdll.spmm_last_error().decode() in str(e.value)


def test_no_rows_is_no_launch(built):
    """R == 0 returns 0 before anything is dereferenced or launched: null arrays, no GPU needed."""
    from spmm_amd._lib import lib
    lib().call("spmm_logit_warp", *_args(lc=None, lu=None, out=None, R=0))
    lib().call("spmm_logit_warp", *_args(R=0))


def test_the_header_declares_and_the_library_exports_the_entry_point(built):
    from spmm_amd._lib import lib, parse_header
    res, argtypes = parse_header()["spmm_logit_warp"]
    assert res is ctypes.c_int and len(argtypes) == 13
    assert argtypes[:5] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int]
    assert argtypes[5:10] == [ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_int]
    assert argtypes[10:] == [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    assert hasattr(lib().cdll, "spmm_logit_warp")
    with open(os.path.join(ROOT, "include", "spmm_hip.h")) as f:
        assert "int spmm_logit_warp(const float* lc, const float* lu, long ld, int R, int V, float w, float temperature, int top_k, float top_p," in f.read()


def test_the_wrapper_passes_the_header_s_prototype():
    """ops.logit_warp in dry-run mode: the argument list matches the header, in place by default."""
    import torch
    from spmm_amd import ops
    lc, lu = torch.zeros(4, 300), torch.zeros(4, 300)
    ops._DRY_RUN, ops._dry_log[:] = True, []
    try:
        assert ops.logit_warp(lc, lu, w=2.0, temperature=0.8, top_k=20, top_p=0.9, min_keep=2) is lc
        both = torch.zeros(8, 300)
        assert ops.logit_warp(both[:4], both[4:], w=2.0, min_keep=2).data_ptr() == both.data_ptr()
    finally:
        ops._DRY_RUN = False
    assert ops._dry_log == ["spmm_logit_warp", "spmm_logit_warp"]
