"""spmm_wordpiece's argument checks (csrc/tokenize.hip), exercised where there is no GPU: every call below is one the entry point refuses
BEFORE a launch -- never add a case here that is complete (this file also runs where there is a GPU).  Also: the header's prototype, the
wrapper's argument list in dry-run mode, and the drivers' choice of the host tokenizer where there is no GPU."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P_ = 0x1000       # "some non-null, 16-byte aligned pointer": never dereferenced


@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return so


def _args(blob=P_, offsets=P_, N=5, gap=1, head=P_, head_len=5, table=P_, table_words=2939, max_chars=250, max_pieces=98, unk_id=1, sep_id=3,
          pad_id=0, ids=P_, ld=99, lens=P_, status=P_):
    return (blob, offsets, N, gap, head, head_len, table, table_words, max_chars, max_pieces, unk_id, sep_id, pad_id, ids, ld, lens, status, None)


REQUIRED = "blob, offsets, table, ids, lens and status are required"
MISALIGNED = r"misaligned table / ids / lens / status \(4 bytes\)"
REFUSED = [
    (_args(N=-1), r"N=-1 \(N >= 0\)"),
    (_args(gap=2), r"gap=2 \(0 or 1\)"),
    (_args(gap=-1), r"gap=-1 \(0 or 1\)"),
    (_args(head_len=-1), r"head_len=-1 \(0 <= head_len <= 16\)"),
    (_args(head_len=17), r"head_len=17 \(0 <= head_len <= 16\)"),
    (_args(max_chars=0), r"max_chars=0 \(1 <= max_chars <= 256\)"),
    (_args(max_chars=257), r"max_chars=257 \(1 <= max_chars <= 256\)"),
    (_args(max_pieces=0, ld=4), r"max_pieces=0 \(max_pieces >= 1\)"),
    (_args(ld=98), r"ld=98 must be >= max_pieces \+ 1 = 99"),
    (_args(max_pieces=148, ld=148), r"ld=148 must be >= max_pieces \+ 1 = 149"),
    (_args(table_words=7), r"table_words=7 \(8 <= table_words <= 8192\)"),
    (_args(table_words=8193), r"table_words=8193 \(8 <= table_words <= 8192\)"),
    (_args(blob=None), REQUIRED),
    (_args(offsets=None), REQUIRED),
    (_args(table=None), REQUIRED),
    (_args(ids=None), REQUIRED),
    (_args(lens=None), REQUIRED),
    (_args(status=None), REQUIRED),
    (_args(head=None), "head is required with head_len=5"),
    (_args(table=P_ + 2), MISALIGNED),
    (_args(ids=P_ + 1), MISALIGNED),
    (_args(lens=P_ + 2), MISALIGNED),
    (_args(status=P_ + 3), MISALIGNED),
    (_args(offsets=P_ + 4), r"misaligned offsets \(8 bytes\)"),
    (_args(N=0, gap=3), "gap=3"),                                   # N == 0 skips the launch, not the checks of the arguments
    (_args(N=0, table_words=0), "table_words=0"),
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[1][:24].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_wordpiece_refuses_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument, with spmm_last_error set; "launch failed" (rc = 2) on a machine
    without a GPU would mean the call got as far as the launch."""
    from spmm_amd._lib import lib
    args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_wordpiece", *args)
    assert "spmm_wordpiece failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert "spmm_wordpiece:" in str(e.value)
    assert lib().cdll.spmm_last_error().decode() in str(e.value)


def test_no_strings_is_no_launch(built):
    """N == 0 returns 0 before anything is dereferenced or launched: null arrays, no GPU needed."""
    from spmm_amd._lib import lib
    lib().call("spmm_wordpiece", *_args(N=0, blob=None, offsets=None, head=None, table=None, ids=None, lens=None, status=None))
    lib().call("spmm_wordpiece", *_args(N=0))


def test_the_header_declares_and_the_library_exports_the_entry_point(built):
    from spmm_amd._lib import lib, parse_header
    res, argtypes = parse_header()["spmm_wordpiece"]
    i, l, p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert res is ctypes.c_int and argtypes == [p, p, i, i, p, i, p, i, i, i, i, i, i, p, l, p, p, p]
    assert hasattr(lib().cdll, "spmm_wordpiece")
    with open(os.path.join(ROOT, "include", "spmm_hip.h")) as f:
        src = f.read()
    assert "int spmm_wordpiece(const unsigned char* blob, const long* offsets, int N, int gap, const unsigned char* head, int head_len," in src
    with open(os.path.join(ROOT, "spmm_amd", "csrc", "Makefile")) as f:
        assert "tokenize.hip" in f.read()


def test_the_constants_of_the_kernel_and_the_host_agree():
    from spmm_amd import ops, wordpiece_device as W
    with open(os.path.join(ROOT, "spmm_amd", "csrc", "tokenize.hip")) as f:
        src = f.read()
    line = "constexpr int TOK_MAGIC = 0x%08X, TOK_TABLE_MAX = %d, TOK_NODES_MAX = %d, TOK_PIECE_MAX = %d, TOK_CHARS_MAX = %d, TOK_HEAD_MAX = %d;" % (
        W.MAGIC, W.TABLE_MAX, W.NODES_MAX, W.PIECE_MAX, W.CHARS_MAX, ops.WORDPIECE_HEAD_MAX)
    assert line in src
    assert (ops.WORDPIECE_TABLE_MAX, ops.WORDPIECE_CHARS_MAX) == (W.TABLE_MAX, W.CHARS_MAX) and len(W.HEAD) <= ops.WORDPIECE_HEAD_MAX


def test_the_wrapper_passes_the_header_s_prototype():
    """ops.wordpiece in dry-run mode: the argument list matches the header; a row-strided ids view passes, wrong dtypes do not."""
    import torch
    from spmm_amd import ops
    blob, off = torch.zeros(40, dtype=torch.uint8), torch.zeros(6, dtype=torch.int64)
    table, head = torch.zeros(2939, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8)
    ids, lens, status = torch.zeros(5, 120, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    kw = dict(gap=1, max_chars=250, max_pieces=98, unk_id=1, sep_id=3, pad_id=0)
    ops._DRY_RUN, ops._dry_log[:] = True, []
    try:
        assert ops.wordpiece(blob, off, table, head, ids, lens, status, **kw) is ids
        ops.wordpiece(blob, off, table, head, ids[:, :99], lens, status, **kw)
        with pytest.raises(AssertionError):
            ops.wordpiece(blob, off.int(), table, head, ids, lens, status, **kw)
        with pytest.raises(AssertionError):
            ops.wordpiece(blob, off, table, head, ids[:, :98], lens, status, **kw)
        with pytest.raises(AssertionError):
            ops.wordpiece(blob, off, table, head, ids.long(), lens, status, **kw)
        with pytest.raises(AssertionError):
            ops.wordpiece(blob, off, torch.zeros(8193, dtype=torch.int32), head, ids, lens, status, **kw)
        with pytest.raises(AssertionError):
            ops.wordpiece(blob, off, table, head, ids, lens[:4], status, **kw)
    finally:
        ops._DRY_RUN = False
    assert ops._dry_log == ["spmm_wordpiece", "spmm_wordpiece"]


# ------------------------------------------------------------------------------------------------------------ the drivers without a GPU
DRIVERS = ["retrieve", "score", "attend", "smiles2pv", "rxn_predict"]


@pytest.mark.parametrize("name", DRIVERS)
def test_the_drivers_parse_the_tokenizer_flags(name):
    import importlib
    mod = importlib.import_module(name)
    assert mod.parse_args(["--host_tokenizer"]).host_tokenizer is True
    assert mod.parse_args([]).host_tokenizer is False


def test_without_a_gpu_the_library_is_tokenised_on_the_host():
    """The holder the drivers batch from: on a CPU device -- with and without --host_tokenizer -- the rows are SmilesWordPiece's own."""
    import numpy as np
    from spmm_amd import wordpiece_device as W
    from spmm_amd.tokenizer import SmilesWordPiece, encode_smiles
    g = np.load(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz"), allow_pickle=False)
    tok = SmilesWordPiece([str(v) for v in g["vocab"]])
    strings = [str(s) for s in g["smiles"]]
    for host_flag in (False, True):
        dev = W.device_tokenizer_for(tok, "cpu", host_flag)
        assert dev is None
        lib = W.TokenLibrary.from_strings(tok, strings, device=dev)
        assert not lib.on_device and lib.rows == encode_smiles(tok, strings)
    import smiles2pv
    seen = []

    def predict(model, ids, mask, n_props):
        import torch
        seen.append((ids.dtype, ids.device.type, tuple(ids.shape)))
        return torch.zeros(ids.shape[0], n_props)

    out = smiles2pv.predict_all(None, tok, strings, 8, predict=predict)
    import torch
    assert tuple(out.shape) == (len(strings), 53) and len(seen) == 3 and all(dt == torch.int64 and dev == "cpu" for dt, dev, _ in seen)
