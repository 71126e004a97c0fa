"""spmm_smiles_mask's argument checks (csrc/syntax.hip), exercised where there is no GPU: every call below is one the entry point refuses
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


def _args(logits=P_, logits2=P_, ld=304, R=6, V=300, tokens=P_, tok_ld=43, hist_rows=6, k=2, mol=None, Lmax=43, t=5, t_ptr=None, t_off=0, t_last=41,
          table=P_, state_out=None):
    return (logits, logits2, ld, R, V, tokens, tok_ld, hist_rows, k, mol, Lmax, t, t_ptr, t_off, t_last, table, state_out, None)


REQUIRED = "logits, tokens and table are required"
MISALIGNED = r"misaligned logits / logits2 / tokens / mol / t_ptr / state_out \(4 bytes\)"
REFUSED = [
    (_args(logits=None), REQUIRED),
    (_args(tokens=None), REQUIRED),
    (_args(table=None), REQUIRED),
    (_args(R=-2), r"R=-2 \(R >= 0\)"),
    (_args(V=0), r"V=0 \(1 <= V <= 512\)"),
    (_args(V=513, ld=600), r"V=513 \(1 <= V <= 512\)"),
    (_args(k=0), r"k=0 R=6 \(1 <= k <= 8, R a multiple of k\)"),
    (_args(k=9, R=9, hist_rows=9), "k=9 R=9"),
    (_args(k=4), "k=4 R=6"),
    (_args(Lmax=257, t_last=41), r"Lmax=257 \(2 <= Lmax <= 256\)"),
    (_args(Lmax=1, t_last=0), r"Lmax=1 \(2 <= Lmax <= 256\)"),
    (_args(t_last=43), r"t_last=43 Lmax=43 \(0 < t_last < Lmax\)"),
    (_args(t_last=0, t=0), "t_last=0 Lmax=43"),
    (_args(t=0), r"t=0 t_last=41 \(0 < t <= t_last\)"),
    (_args(t=42), "t=42 t_last=41"),
    (_args(t=-3), "t=-3 t_last=41"),
    (_args(ld=299), "ld=299 must be >= V=300"),
    (_args(tok_ld=0), r"tok_ld=0 hist_rows=6 \(both >= 1\)"),
    (_args(hist_rows=0), "tok_ld=43 hist_rows=0"),
    (_args(hist_rows=4), "hist_rows=4 < R=6 without mol"),
    (_args(logits=P_ + 2), MISALIGNED),
    (_args(logits2=P_ + 1), MISALIGNED),
    (_args(tokens=P_ + 2), MISALIGNED),
    (_args(mol=P_ + 3, hist_rows=4), MISALIGNED),
    (_args(t_ptr=P_ + 2, t=0), MISALIGNED),
    (_args(state_out=P_ + 1), MISALIGNED),
    (_args(table=P_ + 4), r"misaligned table \(16 bytes\)"),
    (_args(R=0, V=0), "V=0"),                                      # R == 0 skips the launch, not the checks of the arguments
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[1][:24].replace(' ', '_')}" for i, r in enumerate(REFUSED)])
def test_smiles_mask_refuses_bad_arguments(built, i):
    """A SHAPE error (rc = 1) that names the entry point and the argument, with spmm_last_error set; "launch failed" (rc = 2) on a machine
    without a GPU would mean the call got as far as the launch."""
    from spmm_amd._lib import lib
    args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_smiles_mask", *args)
    assert "spmm_smiles_mask failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert "spmm_smiles_mask:" in str(e.value)
    assert lib().cdll.spmm_last_error().decode() in str(e.value)


def test_no_rows_is_no_launch(built):
    """R == 0 returns 0 before anything is dereferenced or launched: null arrays, no GPU needed."""
    from spmm_amd._lib import lib
    lib().call("spmm_smiles_mask", *_args(logits=None, logits2=None, tokens=None, table=None, R=0))
    lib().call("spmm_smiles_mask", *_args(R=0))
    lib().call("spmm_smiles_mask", *_args(R=0, t=0, t_ptr=P_))


def test_the_header_declares_and_the_library_exports_the_entry_point(built):
    from spmm_amd._lib import lib, parse_header
    res, argtypes = parse_header()["spmm_smiles_mask"]
    i, l, p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert res is ctypes.c_int and argtypes == [p, p, l, i, i, p, l, i, i, p, i, i, p, i, i, p, p, p]
    assert hasattr(lib().cdll, "spmm_smiles_mask")
    with open(os.path.join(ROOT, "include", "spmm_hip.h")) as f:
        src = f.read()
    assert "int spmm_smiles_mask(float* logits, float* logits2, long ld, int R, int V, const int* tokens, long tok_ld, int hist_rows, int k," in src
    assert "#define SPMM_SYNTAX_MASKED (-1e30f)" in src


def test_the_wrapper_passes_the_header_s_prototype():
    """ops.smiles_mask in dry-run mode: the argument list matches the header; a 3-D book history and the strided first-pick view pass."""
    import torch
    from spmm_amd import ops
    logits, table = torch.zeros(8, 300), torch.zeros(300, 4, dtype=torch.int32)
    tokens = torch.zeros(4, 2, 43, dtype=torch.int32)
    ops._DRY_RUN, ops._dry_log[:] = True, []
    try:
        assert ops.smiles_mask(logits, tokens, table, t=3, t_last=41, k=2) is logits
        ops.smiles_mask(logits[:4], tokens[:, 0], table, t=1, t_last=41, k=1, logits2=logits[4:], Lmax=43)
        with pytest.raises(AssertionError):
            ops.smiles_mask(logits, tokens.long(), table, t=3, t_last=41, k=2)
        with pytest.raises(AssertionError):
            ops.smiles_mask(logits, tokens, table[:299], t=3, t_last=41, k=2)
    finally:
        ops._DRY_RUN = False
    assert ops._dry_log == ["spmm_smiles_mask", "spmm_smiles_mask"]
