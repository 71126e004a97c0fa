"""The argument checks of csrc/neighbors.hip's entry points, exercised where there is no GPU: every call below is one the entry point refuses
BEFORE a launch -- never add a case here that is complete (this file also runs where there is a GPU)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P_ = 0x1000       # "some non-null, 16-byte aligned pointer": never dereferenced
Q_ = 0x2000


@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return so


def _range(f=P_, ldf=256, r0=0, n=100, c=P_, ldc=256, c0=0, nc=100, E=256, threshold=0.5, counts=P_, offsets=None, nbr=None, nbr_len=0):
    return (f, ldf, r0, n, c, ldc, c0, nc, E, threshold, counts, offsets, nbr, nbr_len, None)


def _round(counts=P_, offsets=P_, nbr=P_, nbr_len=10, n=100, by_count=1, state_in=P_, state_out=Q_, open_out=P_):
    return (counts, offsets, nbr, nbr_len, n, by_count, state_in, state_out, open_out, None)


def _finish(counts=P_, offsets=P_, nbr=P_, nbr_len=10, n=100, by_count=1, state=P_, leader=Q_):
    return (counts, offsets, nbr, nbr_len, n, by_count, state, leader, None)


REFUSED = [
    ("spmm_sim_range", _range(E=96), "E=96 must be a multiple of 64 up to 512"),
    ("spmm_sim_range", _range(E=576), "E=576 must be a multiple of 64 up to 512"),
    ("spmm_sim_range", _range(E=0), "E=0 must be a multiple of 64 up to 512"),
    ("spmm_sim_range", _range(n=-1), "n=-1 must be in"),
    ("spmm_sim_range", _range(n=2 ** 31 - 255), r"n=2147483393 must be in \[0, 2\^31 - 256\]"),
    ("spmm_sim_range", _range(nc=-1), "nc=-1 must be in"),
    ("spmm_sim_range", _range(nc=2 ** 31 - 255), r"nc=2147483393 must be in \[0, 2\^31 - 256\]"),
    ("spmm_sim_range", _range(r0=-1), "r0=-1 with n=100 must keep row indices"),
    ("spmm_sim_range", _range(r0=2 ** 31 - 100), "r0=2147483548 with n=100 must keep row indices"),
    ("spmm_sim_range", _range(c0=-1), "c0=-1 with nc=100 must keep column indices"),
    ("spmm_sim_range", _range(c0=2 ** 31 - 100), "c0=2147483548 with nc=100 must keep column indices"),
    ("spmm_sim_range", _range(threshold=float("nan")), "threshold is NaN"),
    ("spmm_sim_range", _range(nbr_len=-1), "nbr_len=-1 must be at least 0"),
    ("spmm_sim_range", _range(offsets=P_), "offsets, nbr and nbr_len come together"),
    ("spmm_sim_range", _range(nbr=P_, nbr_len=8), "offsets, nbr and nbr_len come together"),
    ("spmm_sim_range", _range(nbr_len=8), "offsets, nbr and nbr_len come together"),
    ("spmm_sim_range", _range(offsets=P_ + 4, nbr=P_, nbr_len=8), "misaligned offsets / nbr"),
    ("spmm_sim_range", _range(offsets=P_, nbr=P_ + 2, nbr_len=8), "misaligned offsets / nbr"),
    ("spmm_sim_range", _range(counts=None), "null counts"),
    ("spmm_sim_range", _range(counts=P_ + 2), "misaligned counts"),
    ("spmm_sim_range", _range(f=None), "null f / c"),
    ("spmm_sim_range", _range(c=None), "null f / c"),
    ("spmm_sim_range", _range(f=P_ + 4), "f / c must be 16-byte aligned"),
    ("spmm_sim_range", _range(c=P_ + 8), "f / c must be 16-byte aligned"),
    ("spmm_sim_range", _range(ldf=258), "ldf=258 ldc=256 must be multiples of 4"),
    ("spmm_sim_range", _range(ldc=255), "ldf=256 ldc=255 must be multiples of 4"),
    ("spmm_sim_range", _range(ldc=128), "ldf=256 ldc=128 must be multiples of 4, at least E=256"),
    ("spmm_leader_round", _round(n=-1), "n=-1 must be in"),
    ("spmm_leader_round", _round(n=2 ** 31), "must be in"),
    ("spmm_leader_round", _round(nbr_len=-1), "nbr_len=-1 must be at least 0"),
    ("spmm_leader_round", _round(by_count=2), "by_count=2 must be 0 or 1"),
    ("spmm_leader_round", _round(by_count=-1), "by_count=-1 must be 0 or 1"),
    ("spmm_leader_round", _round(counts=None), "null counts with by_count=1"),
    ("spmm_leader_round", _round(offsets=None), "null offsets / nbr / state_in / state_out / open_out"),
    ("spmm_leader_round", _round(nbr=None), "null offsets / nbr / state_in / state_out / open_out"),
    ("spmm_leader_round", _round(state_in=None), "null offsets / nbr / state_in / state_out / open_out"),
    ("spmm_leader_round", _round(state_out=None), "null offsets / nbr / state_in / state_out / open_out"),
    ("spmm_leader_round", _round(open_out=None), "null offsets / nbr / state_in / state_out / open_out"),
    ("spmm_leader_round", _round(state_out=P_), "state_in and state_out must be two buffers"),
    ("spmm_leader_round", _round(offsets=P_ + 4), "misaligned pointer"),
    ("spmm_leader_round", _round(state_out=Q_ + 2), "misaligned pointer"),
    ("spmm_leader_finish", _finish(n=-1), "n=-1 must be in"),
    ("spmm_leader_finish", _finish(nbr_len=-1), "nbr_len=-1 must be at least 0"),
    ("spmm_leader_finish", _finish(by_count=3), "by_count=3 must be 0 or 1"),
    ("spmm_leader_finish", _finish(counts=None), "null counts with by_count=1"),
    ("spmm_leader_finish", _finish(offsets=None), "null offsets / nbr / state / leader"),
    ("spmm_leader_finish", _finish(nbr=None), "null offsets / nbr / state / leader"),
    ("spmm_leader_finish", _finish(state=None), "null offsets / nbr / state / leader"),
    ("spmm_leader_finish", _finish(leader=None), "null offsets / nbr / state / leader"),
    ("spmm_leader_finish", _finish(leader=Q_ + 2), "misaligned pointer"),
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[0][5:]}-{r[2][:20].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_neighbour_entry_points_refuse_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument; "launch failed" (rc = 2) on a machine without a GPU would mean
    the call got as far as the launch."""
    from spmm_amd._lib import lib
    name, args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call(name, *args)
    assert f"{name} failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert f"{name}:" in str(e.value)


def test_no_rows_or_no_columns_is_a_no_op(built):
    """n = 0 / nc = 0 return before any data pointer is looked at (and before any launch)."""
    from spmm_amd._lib import lib
    lib().call("spmm_sim_range", *_range(n=0, f=None, counts=None))
    lib().call("spmm_sim_range", *_range(nc=0, c=None))
    lib().call("spmm_leader_round", *_round(n=0))
    lib().call("spmm_leader_finish", *_finish(n=0))


def test_the_header_declares_the_entry_points():
    """_lib resolves what include/spmm_hip.h declares: the three prototypes are parsed with the argument lists of the .hip definitions."""
    import ctypes
    from spmm_amd._lib import parse_header
    protos = parse_header()
    V, L, I, F = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
    assert protos["spmm_sim_range"] == (I, [V, L, L, L, V, L, L, L, I, F, V, V, V, L, V])
    assert protos["spmm_leader_round"] == (I, [V, V, V, L, L, I, V, V, V, V])
    assert protos["spmm_leader_finish"] == (I, [V, V, V, L, L, I, V, V, V])
