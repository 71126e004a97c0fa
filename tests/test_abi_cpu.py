"""CPU-side checks of the C-ABI boundary: the shared library loads and exports exactly what include/spmm_hip.h declares.
No compute call is made (there is no GPU in the dev container)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    so = os.path.join(ROOT, "spmm_amd", "libspmm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return so


def test_library_exports_every_declared_symbol(built):
    from spmm_amd import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 30
    cdll = ctypes.CDLL(built)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/spmm_hip.h but not exported"
    # and nothing spmm_* is exported that the header does not declare
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("spmm_")}
    assert exported - {"spmm_set_error"} == set(protos), exported ^ set(protos)


def test_version_and_error_channel(built):
    from spmm_amd._lib import lib
    L = lib()
    assert L.cdll.spmm_version() == 100
    assert isinstance(L.cdll.spmm_last_error(), bytes)


def test_bad_shape_is_reported_without_touching_the_gpu(built):
    """Argument validation happens before any launch, so it can be exercised on a CPU-only box."""
    from spmm_amd._lib import lib
    L = lib()
    with pytest.raises(RuntimeError, match="multiple of 64"):
        L.call("spmm_gemm_nt", None, 8, None, 8, 16, 16, 100, 1, None, None, 1.0, None, 0, None, 0, None, 16, None, 0, 0, None, 0, None, None)
    with pytest.raises(RuntimeError, match=r"must be in \[1,256\]"):
        L.call("spmm_attn_fwd", None, 64, None, 64, None, 64, None, None, None, None, None, None, None, 64, None, 1, 1, 300, 54, 1, 0, 0.0, None, 0, 0, 0, None)
    with pytest.raises(RuntimeError, match="SPMM_models.py:279"):
        L.call("spmm_enqueue", None, 5, 64, None, 16, None, None, 64, 4, None, 1, None, None)


# Stands for "some non-null pointer" in calls that are refused before any launch (never dereferenced).  This file also runs where there
# is a GPU: every call below must stay one that its entry point refuses BEFORE the launch -- never add a case here that is complete.
P_ = 0x1000


def _embed_fwd_args(mode=0, ids=P_, word=P_, pos=P_, type0=P_, pv_x=P_, pv_mask=P_, pv_w=P_, pv_b=P_, pv_cls=P_, pv_masktok=P_, src_mod=1,
                    gamma=P_, beta=P_, y=P_, zout=None, mean=None, rstd=None, nseq=2, L=3, H=128):
    return (mode, ids, word, pos, type0, pv_x, pv_mask, pv_w, pv_b, pv_cls, pv_masktok, src_mod, gamma, beta, y, zout, mean, rstd, nseq, L, H,
            1e-12, 0.0, None, 0, None)


def _embed_bwd_args(mode=0, dz=P_, ids=P_, pv_x=P_, pv_mask=P_, src_mod=1, dword=P_, dpos=P_, dtype0=P_, d_w=P_, d_b=P_, d_cls=P_, d_masktok=P_):
    return (mode, dz, ids, pv_x, pv_mask, src_mod, dword, dpos, dtype0, d_w, d_b, d_cls, d_masktok, 2, 3, 128, None)


def _ln_fwd_args(x=P_, gamma=P_, beta=P_, y=P_, mean=None, rstd=None):
    return (x, None, gamma, beta, y, None, mean, rstd, 4, 128, 1e-12, 0.0, None, 0, None, None)


# every call is complete except for the one thing named: (entry point, arguments, what the message must say)
REFUSED = (
    [("spmm_embed_bwd", _embed_bwd_args(0, **{k: None}), "mode 0 needs ids and dword") for k in ("ids", "dword")]
    + [("spmm_embed_bwd", _embed_bwd_args(1, **{k: None}), "mode 1 needs pv_x, pv_mask") for k in ("pv_x", "pv_mask", "d_w", "d_b", "d_cls", "d_masktok")]
    + [("spmm_embed_bwd", _embed_bwd_args(1, src_mod=sm), r"src_mod=-?\d") for sm in (0, -3)]
    + [("spmm_embed_bwd", _embed_bwd_args(md), rf"spmm_embed_bwd: mode {md} ") for md in (2, -1, 3)]
    + [("spmm_embed_bwd", _embed_bwd_args(md, **{k: None}), "spmm_embed_bwd: null dz / dpos / dtype0") for md in (0, 1) for k in ("dz", "dpos", "dtype0")]
    + [("spmm_embed_ln_fwd", _embed_fwd_args(md, H=0), "spmm_embed_ln_fwd: nseq=2 L=3 H=0") for md in (0, 1, 2)]
    + [("spmm_embed_ln_fwd", _embed_fwd_args(md, **{k: None}), "spmm_embed_ln_fwd: null pos / type0 / gamma / beta / y")
       for md in (0, 2) for k in ("pos", "type0", "gamma", "beta", "y")]
    + [("spmm_embed_ln_fwd", _embed_fwd_args(0, mean=P_), "spmm_embed_ln_fwd: mean and rstd come together"),
       ("spmm_embed_ln_fwd", _embed_fwd_args(1, rstd=P_), "spmm_embed_ln_fwd: mean and rstd come together"),
       ("spmm_embed_ln_fwd", _embed_fwd_args(3), "spmm_embed_ln_fwd: unknown mode 3"),
       ("spmm_embed_ln_fwd", _embed_fwd_args(0, word=None), "missing inputs for mode 0"),
       ("spmm_embed_ln_fwd", _embed_fwd_args(1, pv_cls=None), "missing inputs for mode 1"),
       ("spmm_embed_ln_fwd", _embed_fwd_args(1, src_mod=0), "missing inputs for mode 1"),
       ("spmm_embed_ln_fwd", _embed_fwd_args(2, pv_x=None), "missing inputs for mode 2"),
       ("spmm_ln_fwd", _ln_fwd_args(mean=P_), "spmm_ln_fwd: mean and rstd come together"),
       ("spmm_ln_fwd", _ln_fwd_args(rstd=P_), "spmm_ln_fwd: mean and rstd come together")]
    + [("spmm_ln_fwd", _ln_fwd_args(**{k: None}), "spmm_ln_fwd: null x / gamma / beta / y") for k in ("x", "gamma", "beta", "y")]
    + [("spmm_ln_bwd", tuple(None if i == k else a for i, a in enumerate((P_, None, P_, P_, P_, P_, P_, None, None, None, 4, 128, 0.0, None, 0, 0, None, None,
                                                                          None, None))), "spmm_ln_bwd: null dy / z / rstd / gamma / dz")
       for k in (0, 2, 4, 5, 6)]
    + [("spmm_transpose_bf16", (P_, 39, P_, 64, 60, 40, 64, None, None), "spmm_transpose_bf16: ldi=39 is shorter than a row of C=40"),
       ("spmm_transpose_bf16", (None, 40, P_, 64, 60, 40, 64, None, None), "spmm_transpose_bf16: null in / out"),
       ("spmm_transpose_bf16", (P_, 40, None, 64, 60, 40, 64, None, None), "spmm_transpose_bf16: null in / out"),
       ("spmm_segment_sum_bf16", (None, P_, P_, P_, 3, 64, None), "spmm_segment_sum_bf16: null src / start / list / out"),
       ("spmm_segment_sum_bf16", (P_, None, P_, P_, 3, 64, None), "spmm_segment_sum_bf16: null src / start / list / out"),
       ("spmm_segment_sum_bf16", (P_, P_, None, P_, 3, 64, None), "spmm_segment_sum_bf16: null src / start / list / out"),
       ("spmm_segment_sum_bf16", (P_, P_, P_, None, 3, 64, None), "spmm_segment_sum_bf16: null src / start / list / out"),
       ("spmm_acc_rows", (None, 128, P_, 128, None, 5, 128, 0, None), "spmm_acc_rows: null dst / src"),
       ("spmm_acc_rows", (P_, 128, None, 128, None, 5, 128, 1, None), "spmm_acc_rows: null dst / src"),
       ("spmm_acc_rows", (P_, 64, P_, 128, None, 5, 128, 0, None), "spmm_acc_rows: ldd=64 lds=128 are shorter"),
       ("spmm_cast_transpose", (None, P_, P_, 4, 5, None), "spmm_cast_transpose: null in, or neither out nor outT"),
       ("spmm_cast_transpose", (P_, None, None, 4, 5, None), "spmm_cast_transpose: null in, or neither out nor outT"),
       ("spmm_cast_f32_bf16", (None, P_, 8, None), "spmm_cast_f32_bf16: null in / out"),
       ("spmm_cast_bf16_f32", (P_, None, 8, None), "spmm_cast_bf16_f32: null in / out"),
       ("spmm_gather_rows", (None, P_, P_, 3, 8, None), "spmm_gather_rows: null dst / src"),
       ("spmm_gather_rows2", (None, P_, None, P_, 3, 8, None), "spmm_gather_rows2: null dst"),
       ("spmm_add_rows_bf16", (P_, P_, None, 3, 8, None), "spmm_add_rows_bf16: null dst / src"),
       ("spmm_gelu_bwd", (P_, None, P_, 8, None), "spmm_gelu_bwd: null dz / pre / out"),
       ("spmm_zero_bytes", (None, 64, None), "spmm_zero_bytes: null p"),
       ("spmm_zero_rows", (None, 3, 16, 48, None), "spmm_zero_rows: null p"),
       ("spmm_zero_rows", (P_, 3, 32, 16, None), "spmm_zero_rows: stride_bytes=16 is shorter than a row of 32 bytes"),
       ("spmm_colsum_bf16", (None, 8, 4, 8, P_, None, None), "spmm_colsum_bf16: null x / out"),
       ("spmm_colsum_bf16", (P_, 8, 4, 8, None, None, None), "spmm_colsum_bf16: null x / out"),
       ("spmm_colsum_bf16", (P_, 8, 4, 12, P_, None, None), "ld=8 shorter than a row of C=12"),
       ("spmm_gemm_tn_reduce", (None, 1, 4, 4, P_, 4, None), "spmm_gemm_tn_reduce: ns=1 N=4 K=4 ldc=4"),
       ("spmm_gemm_tn_reduce", (P_, 1, 4, 8, P_, 4, None), "spmm_gemm_tn_reduce: ldc=4 is shorter than a row of K=8")])


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[0]}" for i, r in enumerate(REFUSED)])
def test_row_kernel_entry_points_refuse_incomplete_calls(built, i):
    """The embedding, LayerNorm-forward, layout and row-helper entry points refuse a call with a missing tensor, an unknown mode or a stride
    shorter than a row as a SHAPE error (rc = 1) that names the entry point and the argument -- before any launch, so this runs anywhere.
    "launch failed" (rc = 2) on a machine without a GPU would mean the call got as far as the launch: a null dereference on a GPU."""
    from spmm_amd._lib import lib
    name, args, msg = REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call(name, *args)
    assert f"{name} failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)
    assert name in str(e.value).split("): ", 1)[1], "the message names its entry point: " + str(e.value)


def _gemm_nt_args(M=256, N=256, K=128, splits=1, R=None, ldr=0, ldc=256, epi=2, colsum=None, kernel=0):
    return (P_, K, P_, K, M, N, K, splits, None, None, 1.0, R, ldr, None, 0, P_, ldc, None, 0, epi, colsum, kernel, None, None)


F32_, ATOMIC_, ACC_ = 2, 3, 5          # SPMM_EPI_F32 / _F32_ATOMIC / _F32_ACC
GEMM_NT_REFUSED = (
    [(_gemm_nt_args(epi=e, kernel=k), "8-phase kernel needs a bf16-output epilogue") for e in (F32_, ATOMIC_, ACC_) for k in (8, 9)]
    + [(_gemm_nt_args(epi=e, kernel=3), "256x256 kernel has bf16-output epilogues only") for e in (F32_, ATOMIC_, ACC_)]
    + [(_gemm_nt_args(epi=ATOMIC_, kernel=2), "256x128 kernel has no atomic epilogue"),
       (_gemm_nt_args(epi=ATOMIC_, kernel=2, splits=2), "256x128 kernel has no atomic epilogue"),
       (_gemm_nt_args(epi=F32_, kernel=2, splits=2), "split-K needs the atomic epilogue"),
       (_gemm_nt_args(epi=0, kernel=2, splits=2), "split-K needs the atomic epilogue")]
    + [(_gemm_nt_args(epi=e, splits=2, kernel=k), "split-K needs the atomic epilogue") for e in (F32_, ACC_) for k in (0, 1, 5)]
    + [(_gemm_nt_args(epi=e, N=258, ldc=260), "N=258 must be a multiple of 4") for e in (F32_, ATOMIC_, ACC_)]
    + [(_gemm_nt_args(epi=e, ldc=258), "ldc must be a multiple of 4") for e in (F32_, ATOMIC_, ACC_)]
    + [(_gemm_nt_args(epi=e, colsum=P_), "colsum is only fused into the bf16") for e in (F32_, ATOMIC_, ACC_)]
    + [(_gemm_nt_args(epi=e, R=P_, ldr=258), "R of an fp32-output epilogue is read 4 columns at a time") for e in (F32_, ATOMIC_, ACC_)]
    + [(_gemm_nt_args(epi=F32_, R=P_ + 4, ldr=256), "R of an fp32-output epilogue is read 4 columns at a time")])


@pytest.mark.parametrize("i", range(len(GEMM_NT_REFUSED)))
def test_gemm_nt_refuses_what_its_fp32_epilogues_do_not_support(built, i):
    """spmm_gemm_nt with an fp32-output epilogue on a kernel that has none (8-phase, 256x256; the 256x128 kernel has no atomic one), split-K
    without the atomic epilogue or on the 256x128 kernel, N or ldc that break the 16-byte stores, fused column sums, an R whose rows are not
    8-byte aligned: each a SHAPE error (rc = 1) before any launch -- the pointers are dummies."""
    from spmm_amd._lib import lib
    args, msg = GEMM_NT_REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_gemm_nt", *args)
    assert "spmm_gemm_nt failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)


def _gemm_tn_args(A=P_, lda=256, B=P_, ldb=256, M=512, N=256, K=256, splits=1, C=P_, ldc=256, ws=P_, kernel=0):
    return (A, lda, B, ldb, M, N, K, splits, 1.0, C, ldc, ws, kernel, None, None)


GEMM_TN_REFUSED = (
    [(_gemm_tn_args(**{k: None}), "spmm_gemm_tn: null A / B / C") for k in ("A", "B", "C")]
    + [(_gemm_tn_args(**{k: 0}), "spmm_gemm_tn: empty problem") for k in ("M", "N", "K")]
    + [(_gemm_tn_args(M=-5), "spmm_gemm_tn: empty problem M=-5"),
       (_gemm_tn_args(N=254), "N=254 K=256 ldc=256 must be multiples of 4"),
       (_gemm_tn_args(K=254), "N=256 K=254 ldc=256 must be multiples of 4"),
       (_gemm_tn_args(ldc=258), "N=256 K=256 ldc=258 must be multiples of 4"),
       (_gemm_tn_args(ldc=252), "spmm_gemm_tn: ldc=252 is shorter than a row of K=256"),
       (_gemm_tn_args(lda=260), "lda=260 / ldb=256 must be multiples of 8"),
       (_gemm_tn_args(ldb=260), "lda=256 / ldb=260 must be multiples of 8"),
       (_gemm_tn_args(lda=248), "lda=248 / ldb=256 must be multiples of 8 covering"),
       (_gemm_tn_args(ldb=248), "lda=256 / ldb=248 must be multiples of 8 covering"),
       (_gemm_tn_args(N=252, lda=252), "lda=252 / ldb=256 must be multiples of 8 covering"),     # the last chunk of N = 252 ends at 256
       (_gemm_tn_args(A=P_ + 8), "spmm_gemm_tn: A/B must be 16-B aligned"),
       (_gemm_tn_args(B=P_ + 2), "spmm_gemm_tn: A/B must be 16-B aligned")]
    + [(_gemm_tn_args(kernel=k), rf"spmm_gemm_tn: unknown kernel selector {k}") for k in (2, 9, -1)]
    + [(_gemm_tn_args(kernel=8, N=260, lda=264), "the 8-phase kernel needs N % 8 == 0 and K % 8 == 0"),
       (_gemm_tn_args(kernel=8, K=260, ldb=264, ldc=260), "the 8-phase kernel needs N % 8 == 0 and K % 8 == 0")]
    + [(_gemm_tn_args(splits=2, ws=None, kernel=k), "spmm_gemm_tn: split reduction needs a workspace") for k in (0, 1, 8)]
    + [(_gemm_tn_args(kernel=8, M=1 << 21, N=1024, K=256, lda=1024), "32-bit byte offsets"),
       (_gemm_tn_args(kernel=8, M=1 << 21, N=256, K=1024, ldb=1024, ldc=1024), "32-bit byte offsets"),
       (_gemm_tn_args(kernel=0, M=1 << 21, N=1024, K=256, lda=1024), "32-bit byte offsets")])


@pytest.mark.parametrize("i", range(len(GEMM_TN_REFUSED)))
def test_gemm_tn_refuses_incomplete_calls(built, i):
    """Every check of spmm_gemm_tn, one call each that is complete but for the thing named: a null A, B or C, an empty problem, N / K / ldc
    that break the 16-byte stores, ldc shorter than a row, lda / ldb that break or do not cover the 16-byte chunks, a misaligned operand,
    an unknown kernel, the 8-phase kernel with N or K % 8 != 0, a split without a workspace, operands past the 8-phase kernel's 32-bit
    offsets: each a SHAPE error (rc = 1) before any launch -- the pointers are dummies."""
    from spmm_amd._lib import lib
    args, msg = GEMM_TN_REFUSED[i]
    with pytest.raises(RuntimeError, match=msg) as e:
        lib().call("spmm_gemm_tn", *args)
    assert "spmm_gemm_tn failed (rc=1)" in str(e.value) and "launch failed" not in str(e.value), str(e.value)


def test_gemm_tn_workspace_and_split_count(built):
    """spmm_gemm_tn_workspace_bytes = splits * N * K * 4 for splits > 1, else 0; spmm_gemm_tn_splits >= 1 at every case of the edge tests,
    and 1 below 2048 rows (at least 16 reduction steps per slice: the training step never reaches the short-M slicing the edge tests force)."""
    import gemm_tn_reference as G
    from spmm_amd._lib import lib
    c = lib().cdll
    for (M, N, K) in ((641, 256, 256), (1000, 300, 132), (1, 4, 4), (16384, 768, 768)):
        assert [c.spmm_gemm_tn_workspace_bytes(M, N, K, s) for s in (-1, 0, 1)] == [0, 0, 0]
        for s in (2, 3, 7, 256):
            assert c.spmm_gemm_tn_workspace_bytes(M, N, K, s) == s * N * K * 4
    for p in G.ALL_CASES:
        for kernel in (p.kernel, 0):
            assert c.spmm_gemm_tn_splits(p.M, p.N, p.K, kernel) == 1, p.name
    assert all(p.M < 2048 for p in G.ALL_CASES)
    for (M, N, K), forced in G.CASES_AUTO:
        assert c.spmm_gemm_tn_splits(M, N, K, 0) == c.spmm_gemm_tn_splits(M, N, K, forced) >= 1
    assert c.spmm_gemm_tn_splits(2047, 768, 768, 8) == 1 and c.spmm_gemm_tn_splits(2048, 768, 768, 8) == 2
    assert c.spmm_gemm_tn_splits(2047, 768, 768, 1) == 1 and c.spmm_gemm_tn_splits(2048, 768, 768, 1) == 2


def test_product_refuses_to_run_without_the_extension(tmp_path):
    """No CPU / eager fallback: with the shared library missing the library handle and the ops that reach it raise and name the file
    they looked for (ops that take a stream fail even earlier on a box without a GPU: torch reports the missing device)."""
    code = (
        "import sys, torch\n"
        "from spmm_amd import _lib, ops\n"
        "for what, fn in (('lib', _lib.lib), ('op', ops.adam_scalars_bytes), ('query', lambda: ops.xattn_supported(768, 12, 54, 128))):\n"
        "    try:\n"
        "        fn()\n"
        "    except RuntimeError as e:\n"
        "        assert 'no CPU / eager fallback' in str(e) and 'missing_lib.so' in str(e), e\n"
        "    else:\n"
        "        sys.exit(what + ' did not raise')\n"
        "print('refused')\n")
    env = dict(os.environ, SPMM_HIP_LIB=str(tmp_path / "missing_lib.so"), PYTHONPATH=ROOT)
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr
