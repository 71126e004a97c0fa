"""The argument checks of csrc/cluster.hip's entry points, exercised where there is no GPU: every call below is one the entry point refuses
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


def _assign(f=P_, ldf=256, c=P_, ldc=256, c0=0, n=100, Kc=8, E=256, best=P_, assign=P_, merge=0, prev=None, changed=None):
    return (f, ldf, c, ldc, c0, n, Kc, E, best, assign, merge, prev, changed, None)


def _group(assign=P_, n=100, K=8, counts=P_, offsets=P_, members=P_, outside=P_, ws=P_, ws_bytes=1 << 20):
    return (assign, n, K, counts, offsets, members, outside, ws, ws_bytes, None)


def _centroids(f=P_, ldf=256, n=100, E=256, best=P_, counts=P_, offsets=P_, members=P_, K=8, centres=P_, ldc=256, norm=P_, medoid=P_, ws=P_,
               ws_bytes=1 << 20):
    return (f, ldf, n, E, best, counts, offsets, members, K, centres, ldc, norm, medoid, ws, ws_bytes, None)


REFUSED = [
    ("spmm_centroid_assign", _assign(E=96), "E=96 must be a multiple of 64 up to 512"),
    ("spmm_centroid_assign", _assign(E=576), "E=576 must be a multiple of 64 up to 512"),
    ("spmm_centroid_assign", _assign(E=0), "E=0 must be a multiple of 64 up to 512"),
    ("spmm_centroid_assign", _assign(Kc=0), "Kc=0 must be at least 1"),
    ("spmm_centroid_assign", _assign(c0=-1), "c0=-1 with Kc=8 must keep centre indices"),
    ("spmm_centroid_assign", _assign(c0=2 ** 31 - 8), "c0=2147483640 with Kc=8 must keep centre indices"),
    ("spmm_centroid_assign", _assign(n=-1), "n=-1 must be in"),
    ("spmm_centroid_assign", _assign(n=2 ** 31 - 255), r"must be in \[0, 2\^31 - 256\]"),
    ("spmm_centroid_assign", _assign(merge=2), "merge=2 must be 0 or 1"),
    ("spmm_centroid_assign", _assign(prev=P_), "prev and changed come together"),
    ("spmm_centroid_assign", _assign(changed=P_), "prev and changed come together"),
    ("spmm_centroid_assign", _assign(prev=P_ + 2, changed=P_), "misaligned prev / changed"),
    ("spmm_centroid_assign", _assign(best=None), "null best / assign"),
    ("spmm_centroid_assign", _assign(assign=None), "null best / assign"),
    ("spmm_centroid_assign", _assign(assign=P_ + 2), "misaligned best / assign"),
    ("spmm_centroid_assign", _assign(f=None), "null f / c"),
    ("spmm_centroid_assign", _assign(c=None), "null f / c"),
    ("spmm_centroid_assign", _assign(f=P_ + 4), "f / c must be 16-byte aligned"),
    ("spmm_centroid_assign", _assign(c=P_ + 8), "f / c must be 16-byte aligned"),
    ("spmm_centroid_assign", _assign(ldf=258), "ldf=258 ldc=256 must be multiples of 4"),
    ("spmm_centroid_assign", _assign(ldc=255), "ldf=256 ldc=255 must be multiples of 4"),
    ("spmm_centroid_assign", _assign(ldc=128), "ldf=256 ldc=128 must be multiples of 4, at least E=256"),
    ("spmm_cluster_group", _group(K=0), r"K=0 must be in \[1, 2\^24\]"),
    ("spmm_cluster_group", _group(K=2 ** 24 + 1), r"K=16777217 must be in \[1, 2\^24\]"),
    ("spmm_cluster_group", _group(n=-1), "n=-1 must be in"),
    ("spmm_cluster_group", _group(n=2 ** 31), "must be in"),
    ("spmm_cluster_group", _group(counts=None), "null counts / offsets / outside"),
    ("spmm_cluster_group", _group(outside=None), "null counts / offsets / outside"),
    ("spmm_cluster_group", _group(offsets=P_ + 4), "misaligned counts / offsets / outside"),
    ("spmm_cluster_group", _group(assign=None), "null assign / members"),
    ("spmm_cluster_group", _group(members=None), "null assign / members"),
    ("spmm_cluster_group", _group(members=P_ + 2), "misaligned assign / members"),
    ("spmm_cluster_group", _group(ws=None), "workspace of"),
    ("spmm_cluster_group", _group(ws=P_ + 8), "workspace of"),
    ("spmm_cluster_group", _group(ws_bytes=8), "workspace of 32 bytes"),
    ("spmm_cluster_centroids", _centroids(E=0), r"E=0 must be in \[1, 512\]"),
    ("spmm_cluster_centroids", _centroids(E=513), r"E=513 must be in \[1, 512\]"),
    ("spmm_cluster_centroids", _centroids(K=0), r"K=0 must be in \[1, 2\^24\]"),
    ("spmm_cluster_centroids", _centroids(n=-1), "n=-1 must be in"),
    ("spmm_cluster_centroids", _centroids(centres=None), "null counts / offsets / centres / norm / medoid"),
    ("spmm_cluster_centroids", _centroids(medoid=None), "null counts / offsets / centres / norm / medoid"),
    ("spmm_cluster_centroids", _centroids(f=None), "null f / best / members"),
    ("spmm_cluster_centroids", _centroids(best=None), "null f / best / members"),
    ("spmm_cluster_centroids", _centroids(ldf=255), "ldf=255 ldc=256 must be at least E=256"),
    ("spmm_cluster_centroids", _centroids(ldc=100), "ldf=256 ldc=100 must be at least E=256"),
    ("spmm_cluster_centroids", _centroids(offsets=P_ + 4), "misaligned pointer"),
    ("spmm_cluster_centroids", _centroids(norm=P_ + 2), "misaligned pointer"),
    ("spmm_cluster_centroids", _centroids(ws=None), "workspace of"),
    ("spmm_cluster_centroids", _centroids(ws_bytes=64), "workspace of"),
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[0][5:]}-{r[2][:20].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_cluster_entry_points_refuse_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument; "launch failed" (rc = 2) on a machine without a GPU would mean
    the call got as far as the launch."""
    from spmm_amd._lib import lib
    name, args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call(name, *args)
    assert f"{name} failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert f"{name}:" in str(e.value)


def test_no_rows_is_a_no_op_for_assign(built):
    """n = 0 returns before any pointer is looked at (and before any launch)."""
    from spmm_amd._lib import lib
    lib().call("spmm_centroid_assign", *_assign(n=0, f=None, best=None, assign=None))


def test_workspace_queries(built):
    from spmm_amd._lib import lib
    L = lib().cdll
    assert L.spmm_cluster_group_workspace_bytes(100, 8) == 32                      # one block of rows: one line of 8 counts
    assert L.spmm_cluster_group_workspace_bytes(5000, 4097) == (5 * 4097 * 4 + 15) // 16 * 16
    assert L.spmm_cluster_group_workspace_bytes(1 << 20, 65536) == 256 * 65536 * 4   # the table is capped at 2^24 entries
    assert L.spmm_cluster_group_workspace_bytes(10, 0) == 0
    pieces = 1000 // 256 + 8
    assert L.spmm_cluster_centroids_workspace_bytes(1000, 8, 256) == (9 * 8 + 15) // 16 * 16 + (pieces * 8 + 15) // 16 * 16 + pieces * 256 * 4
    assert L.spmm_cluster_centroids_workspace_bytes(-1, 8, 256) == 0
