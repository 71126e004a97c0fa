"""Reference, case list and seeded defects for the fp32-output epilogues of spmm_gemm_nt (SPMM_EPI_F32, SPMM_EPI_F32_ACC,
SPMM_EPI_F32_ATOMIC; include/spmm_hip.h).  Plain torch on the CPU; tests/test_gemm_f32_epilogues_gpu.py runs the kernels on these cases
and tests/test_gemm_f32_reference_cpu.py checks this module itself.

    v = alpha * acc / (*div) + bias + R          acc = A[M,K] . W[N,K]^T over the WHOLE K, whatever `splits` is
    SPMM_EPI_F32:  C = v          SPMM_EPI_F32_ACC, SPMM_EPI_F32_ATOMIC:  C = C0 + v

ref() evaluates that in float64 and in float32; the comparison is helpers_gpu.check_ref: |got - ref64| <= max(8 E32, 4 fp32 ulp of the
largest output), E32 the error of the float32 evaluation -- no fixed tolerance.  Inputs are random values already rounded to bf16
(test_kernels_gpu.py::rnd), bias / C0 are fp32 values, *div is the fp32 scalar the kernel reads.

Every output is checked INSIDE a larger buffer (PAD_ROWS more rows, ldc = N + PAD_COLS) filled with SENTINEL: check_output() asserts the
rule on the view [:M, :N] and that every element outside it still holds SENTINEL's bits.  defective() returns that buffer as a kernel with
one known defect would leave it; the CPU test asserts that check_output() rejects every one of them at every case below -- the condition
that keeps the GPU tests from passing a subtly wrong kernel."""
import functools
from dataclasses import dataclass, replace
from typing import Optional

import torch

from helpers_gpu import check_ref

BF = torch.bfloat16
EPI_BF16, EPI_F32, EPI_F32_ATOMIC, EPI_F32_ACC = 0, 2, 3, 5            # spmm_amd.ops.EPI_* (pinned by the CPU test)
EPI_NAME = {EPI_F32: "f32", EPI_F32_ATOMIC: "atomic", EPI_F32_ACC: "acc"}
SENTINEL = -1234.5
PAD_ROWS, PAD_COLS = 3, 12
DIV = 0.07                                                              # the step's temperature


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    """test_kernels_gpu.py::rnd, left on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def ref(A, W, *, bias=None, alpha=1.0, div=None, R=None, C0=None, epi=EPI_F32, dtype=torch.float64):
    """The documented formula of one launch, every operation in `dtype` (float64 or float32)."""
    v = alpha * (A.to(dtype) @ W.to(dtype).t())
    if div is not None:
        v = v / div.to(dtype)
    if bias is not None:
        v = v + bias.to(dtype)
    if R is not None:
        v = v + R.to(dtype)
    return v if epi == EPI_F32 else C0.to(dtype) + v


# ---------------------------------------------------------------------------------------------------------------------
# problems: one per distinct (shape, epilogue, operands); the kernel selector is not part of it (every kernel computes the same thing)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Problem:
    M: int                              # rows computed (the device-side row count where M_launch is set)
    N: int
    K: int
    epi: int
    bias: bool = True
    alpha: float = 0.5
    div: Optional[float] = DIV
    R: bool = False
    splits: int = 1
    layout: str = "dense"               # dense | cls (A = position-0 rows of [B, L, H]) | wslice (W = columns of a wider matrix) | knarrow (K= < widths)
    launches: int = 1                   # launches that add into the same C, each with operands of its own
    c0: str = "rand"                    # accumulating epilogues: what the view holds before the first launch (rand | zero)
    M_launch: Optional[int] = None      # the launch is sized for M_launch rows, *M_dev = M; A holds NaN in rows [M, M_launch)

    @property
    def rows(self):
        return self.M if self.M_launch is None else self.M_launch

    @property
    def ksplit(self):                   # spmm_gemm_nt's slicing: whole 64-wide tiles per slice, no empty slice
        return ((self.K // 64 + max(self.splits, 1) - 1) // max(self.splits, 1)) * 64

    @property
    def nslices(self):
        return (self.K + self.ksplit - 1) // self.ksplit

    @property
    def name(self):
        s = f"{self.M}x{self.N}x{self.K}-{EPI_NAME[self.epi]}"
        s += (f"-R" if self.R else "") + (f"-s{self.splits}" if self.splits > 1 else "") + (f"-{self.layout}" if self.layout != "dense" else "")
        return s + (f"-x{self.launches}" if self.launches > 1 else "") + (f"-of{self.M_launch}" if self.M_launch else "")


CLS_L, CLS_SPARE = 5, 2                 # cls layout: [B + CLS_SPARE, L, H] tokens, the view takes position 0 of the first B sequences


@functools.lru_cache(maxsize=None)
def _bases(M, rows, N, K, layout, launches):
    """Base tensors (CPU, contiguous) the operands are views of: the same for every epilogue of a shape."""
    A, W = [], []
    for l in range(launches):
        if layout == "cls":
            a = rnd((M + CLS_SPARE) * CLS_L, K, seed=100 + l)
        else:
            a = rnd(rows, 2 * K if layout == "knarrow" else K, seed=100 + l)
            a[M:] = float("nan")
        wk = {"wslice": 3 * K, "knarrow": K + 64}.get(layout, K)
        A.append(a)
        W.append(rnd(N, wk, scale=0.05, seed=200 + l))
    return dict(A=A, W=W, bias=rnd(N, seed=300, dtype=torch.float32), R=rnd(rows, N + 4, seed=400), C0=rnd(M, N, seed=500, dtype=torch.float32),
                div=torch.tensor([DIV], dtype=torch.float32))


def bases(p):
    return _bases(p.M, p.rows, p.N, p.K, p.layout, p.launches)


def to_device(x, dev):
    return {k: [t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) for k, v in x.items()}


def operands(p, x, l=0):
    """The tensors of launch l as ops.gemm_nt takes them (views of x = bases(p), on whatever device x is): A, W, keyword arguments."""
    A, W = x["A"][l], x["W"][l]
    if p.layout == "cls":
        A = A.view(-1, CLS_L * p.K)[:p.M, :p.K]                    # row stride L * H
    elif p.layout == "wslice":
        W = W[:, p.K:2 * p.K]
    kw = dict(bias=x["bias"] if p.bias else None, alpha=p.alpha, div=x["div"] if p.div is not None else None,
              R=x["R"][:, :p.N] if p.R else None, epi=p.epi, splits=p.splits)
    if p.layout == "knarrow":
        kw["K"] = p.K
    return A, W, kw


def initial_buffer(p):
    """[rows + PAD_ROWS, N + PAD_COLS] fp32 of SENTINEL; the accumulating epilogues find C0 in [:M, :N].  C of the launch = buf[:rows, :N]."""
    buf = torch.full((p.rows + PAD_ROWS, p.N + PAD_COLS), SENTINEL, dtype=torch.float32)
    if p.epi != EPI_F32:
        buf[:p.M, :p.N] = bases(p)["C0"] if p.c0 == "rand" else 0.0
    return buf


def _launch_terms(p, x, l):
    A, W, kw = operands(p, x, l)
    return A[:p.M, :p.K], W[:, :p.K], kw["bias"], kw["div"], (kw["R"][:p.M] if p.R else None)


@functools.lru_cache(maxsize=None)
def reference(p):
    """(ref64, ref32) of the view [:M, :N] after all launches: computed once per problem, shared, never modified."""
    x, out = bases(p), []
    for dtype in (torch.float64, torch.float32):
        C = initial_buffer(p)[:p.M, :p.N].to(dtype)
        for l in range(p.launches):
            A, W, bias, div, R = _launch_terms(p, x, l)
            C = ref(A, W, bias=bias, alpha=p.alpha, div=div, R=R, C0=C, epi=p.epi, dtype=dtype)
        out.append(C)
    return tuple(out)


def check_output(name, buf, p):
    """buf: the whole padded buffer after the launches (CPU fp32).  The view [:M, :N] passes check_ref; everything else is SENTINEL's bits."""
    ref64, ref32 = reference(p)
    assert buf.dtype == torch.float32 and tuple(buf.shape) == (p.rows + PAD_ROWS, p.N + PAD_COLS) and buf.is_contiguous()
    check_ref(name, buf[:p.M, :p.N], ref64, ref32)
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[:p.M, :p.N] = False
    touched = outside & (buf.view(torch.int32) != torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32))
    assert not touched.any(), f"{name}: {int(touched.sum())} elements outside [:{p.M}, :{p.N}] written; first {touched.nonzero()[0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# seeded defects
# ---------------------------------------------------------------------------------------------------------------------
DEFECTS = ("k_tile_dropped", "last_slice_dropped", "bias_per_slice", "R_per_slice", "ragged_cols_unwritten", "row_past_M_written",
           "div_ignored", "alpha_ignored")


def applicable_defects(p):
    split = p.nslices > 1
    return [d for d in DEFECTS if {"last_slice_dropped": split, "bias_per_slice": split and p.bias, "R_per_slice": split and p.R,
                                   "div_ignored": p.div is not None, "alpha_ignored": p.alpha != 1.0}.get(d, True)]


def defective(kind, p):
    """The padded buffer as a kernel with ONE defect would leave it (kind = None: no defect), computed in fp32 slice by slice the way a
    split launch adds its K-slices:
      k_tile_dropped         the last 64-wide K-tile of (the last launch's) K is never multiplied
      last_slice_dropped     the last K-slice of the split adds nothing
      bias_per_slice         every K-slice adds the bias          R_per_slice: every K-slice adds R
      ragged_cols_unwritten  the last 4-column group of every row is left as it was
      row_past_M_written     row M (the first one past the rows to compute) receives a row of results
      div_ignored            *div is not applied                  alpha_ignored: alpha is not applied"""
    assert kind is None or kind in DEFECTS
    x, f32 = bases(p), torch.float32
    buf = initial_buffer(p)
    C = buf[:p.M, :p.N].clone()
    for l in range(p.launches):
        A, W, bias, div, R = _launch_terms(p, x, l)
        A, W = A.to(f32), W.to(f32)
        kend = p.K - 64 if (kind == "k_tile_dropped" and l == p.launches - 1) else p.K
        add = torch.zeros(p.M, p.N, dtype=f32)
        for s in range(p.nslices):
            if kind == "last_slice_dropped" and s == p.nslices - 1:
                continue
            k0, k1 = s * p.ksplit, min((s + 1) * p.ksplit, kend)
            v = (A[:, k0:k1] @ W[:, k0:k1].t()) if k1 > k0 else torch.zeros(p.M, p.N, dtype=f32)
            if kind != "alpha_ignored":
                v = p.alpha * v
            if div is not None and kind != "div_ignored":
                v = v / div
            if bias is not None and (s == 0 or kind == "bias_per_slice"):
                v = v + bias
            if R is not None and (s == 0 or kind == "R_per_slice"):
                v = v + R.to(f32)
            add = add + v
        C = add if p.epi == EPI_F32 else C + add
    if kind == "ragged_cols_unwritten":
        C[:, p.N - 4:] = buf[:p.M, p.N - 4:p.N]
    buf[:p.M, :p.N] = C
    if kind == "row_past_M_written":
        buf[p.M, :p.N] = C[p.M - 1]
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gemm_f32_epilogues_gpu.py: (problem, kernel selector)
# ---------------------------------------------------------------------------------------------------------------------
F32, ACC, ATOMIC = EPI_F32, EPI_F32_ACC, EPI_F32_ATOMIC
KERNEL_EPIS = [(k, e) for k in (1, 5) for e in (F32, ACC, ATOMIC)] + [(2, F32), (2, ACC)] + [(0, e) for e in (F32, ACC, ATOMIC)]

# a. every kernel and epilogue at ragged shapes: bias, alpha = 0.5, device scalar div
RAGGED_SHAPES = [(1, 4, 64), (127, 44, 128), (129, 132, 192), (257, 300, 256), (513, 300, 320), (255, 128, 768)]
CASES_RAGGED = [(Problem(M, N, K, e), k) for (M, N, K) in RAGGED_SHAPES for (k, e) in KERNEL_EPIS]

# b. R: added exactly once (K = 320: five K-slices at splits = 5)
CASES_R = ([(Problem(129, 132, 320, e, R=True), k) for k in (0, 1, 2, 5) for e in (F32, ACC)]
           + [(Problem(129, 132, 320, ATOMIC, R=True, splits=s), k) for k in (0, 1, 5) for s in (1, 5)])

# c. strided operands (B = 70, L = 5, H = 128)
CASES_STRIDED = [(Problem(70, 132, 128, F32, layout=lay), k) for lay in ("cls", "wslice", "knarrow") for k in (0, 1, 2, 5)]

# d. split-K: slices of 3 + 2 tiles, one tile each, a split count past K / 64 (clamped to 5), the step's 16-way split
CASES_SPLITK = [(Problem(130, 260, K, ATOMIC, splits=s), k) for (K, s) in ((320, 2), (320, 5), (320, 7), (4096, 16)) for k in (0, 1, 5)]

# e. the four call sites through the automatic choice (+ the LM head on the forced 256x128 kernel)
LM_HEAD = Problem(6144, 300, 768, F32, alpha=1.0, div=None)
DFEAT = Problem(128, 256, 4096, ATOMIC, bias=False, alpha=1.0, splits=16, launches=2, c0="zero")
CASES_SITES = [(LM_HEAD, 0), (LM_HEAD, 2), (Problem(5000, 300, 768, F32, alpha=1.0, div=None), 0),
               (Problem(256, 1064, 768, F32, bias=False, alpha=1.0), 0), (DFEAT, 0),
               (Problem(1000, 1536, 768, ACC, bias=False, alpha=1.0, div=None, launches=2), 0)]

# f. device-side row count: sized for 700 rows, *M_dev = 300, NaN in A's rows [300, 700)
CASES_MDEV = [(Problem(300, 132, 128, e, M_launch=700), k) for (k, e) in KERNEL_EPIS if k != 0]

ALL_CASES = CASES_RAGGED + CASES_R + CASES_STRIDED + CASES_SPLITK + CASES_SITES + CASES_MDEV
PROBLEMS = list(dict.fromkeys(p for p, _ in ALL_CASES))                   # distinct, in order


def case_id(case):
    p, k = case
    return f"k{k}-{p.name}"
