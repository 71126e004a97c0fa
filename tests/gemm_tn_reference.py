"""Reference, case lists and seeded defects for the weight-gradient GEMM spmm_gemm_tn (spmm_amd/csrc/gemm_tn.hip, include/spmm_hip.h):

    C[N,K] = C0 + alpha * A[M,N]^T . B[M,K]          reduced over the rows [0, Meff), Meff = min(max(*M_dev, 0), M) under a device-side count

Plain torch on the CPU; tests/test_gemm_tn_edges_gpu.py runs the kernels on these cases and tests/test_gemm_tn_reference_cpu.py checks this
module itself.

ref() evaluates the formula in float64 and in float32.  The float32 evaluation is an fp32 accumulation in plain row order, in 64-row
blocks (one block = one reduction step of either kernel; each block's product is one fp32 matmul, the blocks are added one after the other,
alpha and C0 come last): a summation order any of the launch paths may legitimately have.  The comparison is helpers_gpu.check_ref:
|got - ref64| <= max(8 E32, 4 fp32 ulp of the largest output), E32 the error of that float32 evaluation -- no fixed tolerance, nothing taken
from what a kernel gives.  Inputs are seeded CPU randn values rounded to bf16, C0 is random fp32.

Every operand sits inside a larger buffer: C is the view [:N, :K] of a buffer with PAD_ROWS more rows and ldc = K + PAD_COLS full of
SENTINEL; A and B are column views of wider buffers (lda = roundup8(N) + 16, ldb = roundup8(K) + 8) whose padding columns hold NaN; and
every row past the rows to reduce -- past the device-side count, or past M where the buffers are taller than the launch -- holds NaN in
BOTH operands.  check_output() asserts the rule on the view, that the view is finite, and that every element outside it still holds
SENTINEL's bits.  defective() returns that buffer as a kernel with one known defect would leave it; the CPU test asserts that
check_output() rejects every one of them at every case below -- the condition that keeps the GPU tests from passing a subtly wrong kernel."""
import functools
from dataclasses import dataclass
from typing import Optional

import torch

from helpers_gpu import check_ref

BF = torch.bfloat16
SENTINEL = -1234.5
PAD_ROWS, PAD_COLS = 3, 12
WS_GUARD = 64                           # sentinel floats behind the workspace
NAN = float("nan")


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    """test_kernels_gpu.py::rnd, left on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def ref(A, B, C0, alpha, dtype):
    """C0 + alpha * A^T B with every operation in `dtype` (float64 or float32): 64-row blocks of the reduction in plain row order."""
    acc = torch.zeros(A.shape[1], B.shape[1], dtype=dtype)
    for m0 in range(0, A.shape[0], 64):
        acc = acc + A[m0:m0 + 64].to(dtype).t() @ B[m0:m0 + 64].to(dtype)
    return C0.to(dtype) + alpha * acc


def _ceil(a, b):
    return -(-a // b)


def slicing8(M, splits):
    """The 8-phase kernel's row slices as include/spmm_hip.h states the rule (M >= 128): -> (ns, rlast, ndup, rs).  Slices of
    rs = ceil(ceil(M / 128) / splits) * 128 rows, ns = ceil(M / rs) of them; the last one is the rlast rows that END at row M, and its first
    ndup rows belong to the slice before; a single slice is the (M / 128) * 128 rows that end at row M (the rest: a 128x128 pass)."""
    rs = _ceil(_ceil(M, 128), max(splits, 1)) * 128
    ns = _ceil(M, rs)
    over = ns * rs - M
    if ns == 1:
        return 1, (M // 128) * 128, 0, rs
    return ns, rs - (over // 128) * 128, over % 128, rs


def _cut8(m, splits):
    """Row ranges [beg, end) the slices of slicing8(m, splits) own (overlap rows go to the slice before)."""
    ns, rlast, ndup, rs = slicing8(m, splits)
    if ns == 1:
        return [(0, m)]
    return [(z * rs, (z + 1) * rs) for z in range(ns - 1)] + [(m - rlast + ndup, m)]


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Problem:
    M: int                              # rows the launch is sized for
    N: int
    K: int
    splits: int = 1
    kernel: int = 8                     # the selector passed to spmm_gemm_tn
    alpha: float = 0.5
    count: Optional[int] = None         # *M_dev (None: no device-side row count)
    rows_buf: Optional[int] = None      # rows of the operand buffers when they are taller than the launch

    @property
    def meff(self):                     # rows that are reduced
        return self.M if self.count is None else min(max(self.count, 0), self.M)

    @property
    def rows(self):
        return self.M if self.rows_buf is None else self.rows_buf

    @property
    def lda(self):
        return (self.N + 7) // 8 * 8 + 16

    @property
    def ldb(self):
        return (self.K + 7) // 8 * 8 + 8

    @property
    def ldc(self):
        return self.K + PAD_COLS

    @property
    def name(self):
        s = f"k{self.kernel}-{self.M}x{self.N}x{self.K}-s{self.splits}-a{self.alpha:g}"
        return s + (f"-of{self.rows_buf}" if self.rows_buf else "") + (f"-count{self.count}" if self.count is not None else "")

    @property
    def plan(self):
        """What tn_run launches: -> (kernel that runs the slices, slabs reduced (0: straight into C), the row ranges [beg, end) of the
        rows [0, meff) each slice reduces -- empty slices included)."""
        M, meff, splits = self.M, self.meff, max(self.splits, 1)
        clip = lambda cuts: [(min(b, meff), min(e, meff)) for b, e in cuts]
        if self.kernel == 8 and M >= 128:
            ns = slicing8(M, splits)[0]
            if self.count is not None and (ns == 1 or M < 256):
                return 1, 0, [(0, meff)]                             # the 128x128 kernel under the count, one slice
            if ns == 1:
                return 8, 0, [(0, M)]
            if self.count is None or self.count >= M:
                return 8, ns, _cut8(M, splits)
            cuts = _cut8(max(meff, 256), ns)                         # re-cut on the device with the ns slices the grid has
            assert len(cuts) <= ns
            return 8, ns, clip(cuts) + [(meff, meff)] * (ns - len(cuts))
        rs = _ceil(_ceil(M, 64), splits) * 64
        ns = _ceil(M, rs)
        return 1, (ns if ns > 1 else 0), clip([(z * rs, min((z + 1) * rs, M)) for z in range(ns)])


@functools.lru_cache(maxsize=None)
def _bases(rows, N, K):
    """Finite base tensors (CPU): A [rows, lda] and B [rows, ldb] with NaN in the padding columns only, C0 [N, K] fp32."""
    lda, ldb = (N + 7) // 8 * 8 + 16, (K + 7) // 8 * 8 + 8
    A, B = rnd(rows, lda, seed=14), rnd(rows, ldb, seed=15)
    A[:, N:] = NAN
    B[:, K:] = NAN
    return A, B, rnd(N, K, seed=500, dtype=torch.float32)


def bases(p):
    return _bases(p.rows, p.N, p.K)


def operand_buffers(p):
    """The buffers of problem p as the launch finds them (fresh CPU tensors): Abuf [rows, lda], Bbuf [rows, ldb] with NaN in the padding
    columns and in every row from meff on, Cbuf [N + PAD_ROWS, ldc] of SENTINEL with C0 in [:N, :K].  The launch takes
    A = Abuf[:M, :N], B = Bbuf[:M, :K], C = Cbuf[:N, :K]."""
    A, B, C0 = bases(p)
    A, B = A.clone(), B.clone()
    A[p.meff:] = NAN
    B[p.meff:] = NAN
    return A, B, initial_buffer(p)


def initial_buffer(p):
    buf = torch.full((p.N + PAD_ROWS, p.ldc), SENTINEL, dtype=torch.float32)
    buf[:p.N, :p.K] = bases(p)[2]
    return buf


@functools.lru_cache(maxsize=None)
def _reference(rows, N, K, meff, alpha):
    A, B, C0 = _bases(rows, N, K)
    return tuple(ref(A[:meff, :N], B[:meff, :K], C0, alpha, dt) for dt in (torch.float64, torch.float32))


def reference(p):
    """(ref64, ref32) of the view [:N, :K]: computed once per distinct problem, shared, never modified."""
    return _reference(p.rows, p.N, p.K, p.meff, p.alpha)


def check_output(name, buf, p):
    """buf: the whole padded C buffer after the launch (CPU fp32).  The view [:N, :K] is finite and passes check_ref; everything else is
    SENTINEL's bits."""
    ref64, ref32 = reference(p)
    assert buf.dtype == torch.float32 and tuple(buf.shape) == (p.N + PAD_ROWS, p.ldc) and buf.is_contiguous()
    view = buf[:p.N, :p.K]
    finite = torch.isfinite(view)
    assert finite.all(), f"{name}: {int((~finite).sum())} non-finite elements in C; first {(~finite).nonzero()[0].tolist()}"
    check_ref(name, view, ref64, ref32)
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[:p.N, :p.K] = False
    touched = outside & (buf.view(torch.int32) != torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32))
    assert not touched.any(), f"{name}: {int(touched.sum())} elements outside [:{p.N}, :{p.K}] written; first {touched.nonzero()[0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# seeded defects
# ---------------------------------------------------------------------------------------------------------------------
def defect_rows(m):
    """The reduction rows at which a slicing, masking or remainder mistake would show, of m reduced rows."""
    c = {0, 1, 63, 64, 127, 128, m % 128 - 1, m % 128, m - 129, m - 128, m - 65, m - 64, m - 1}
    return sorted(r for r in c if 0 <= r < m)


def applicable_defects(p):
    """Kinds of defective() that change the result of problem p."""
    m, (_, slabs, _) = p.meff, p.plan
    kinds = [f"{w}:{r}" for r in defect_rows(m) for w in ("row_dropped", "row_twice")]
    kinds += ["step_dropped"] if m > 0 else []
    kinds += ["row_past_count"] if p.count is not None and m < p.rows else []
    kinds += ["alpha_on_c0"] if p.alpha != 1.0 else []
    kinds += ["overwritten"]
    kinds += ["slab_missing", "slab_twice"] if slabs > 1 and m > 0 else []
    kinds += ["n_chunk_clamped"] if p.N >= 16 and m > 0 else []
    kinds += ["k_chunk_clamped"] if p.K >= 16 and m > 0 else []
    kinds += ["transposed"] if p.N == p.K and m > 0 else []
    return kinds + ["pad_column_written", "row_N_written"]


@functools.lru_cache(maxsize=None)
def _acc32(rows, N, K, meff):
    A, B, _ = _bases(rows, N, K)
    return ref(A[:meff, :N], B[:meff, :K], torch.zeros(N, K), 1.0, torch.float32)


def defective(p, kind):
    """The padded C buffer as a kernel with ONE defect would leave it (kind = None: no defect), in fp32:
      row_dropped:r / row_twice:r   reduction row r contributes nothing / twice
      step_dropped                  the last 64 reduced rows (one reduction step) contribute nothing
      row_past_count                the first row past the device-side count is reduced too -- with finite data where the buffers hold NaN
      alpha_on_c0                   alpha scales C0 as well                overwritten: C = alpha * A^T B, C0 lost
      slab_missing / slab_twice     the last slice that has rows is not reduced / the first slice is reduced twice
      n_chunk_clamped               the last 8-column chunk of A's N columns is read from the chunk before it (a clamp that leaked into
                                    stored outputs); k_chunk_clamped: the same for B's K columns
      transposed                    C^T of the product (N == K)
      pad_column_written            one element written at [N - 1, K]      row_N_written: one element written at [N, 0]"""
    assert kind is None or kind in applicable_defects(p), kind
    A, B, C0 = bases(p)
    A32, B32 = A[:, :p.N].float(), B[:, :p.K].float()
    m, what = p.meff, (kind or "").split(":")[0]
    outer = lambda lo, hi: A32[lo:hi].t() @ B32[lo:hi]
    acc = _acc32(p.rows, p.N, p.K, m).clone()
    if what in ("row_dropped", "row_twice"):
        r = int(kind.split(":")[1])
        acc += outer(r, r + 1) * (-1.0 if what == "row_dropped" else 1.0)
    elif what == "step_dropped":
        acc -= outer(max(m - 64, 0), m)
    elif what == "row_past_count":
        acc += outer(m, m + 1)
    elif what in ("slab_missing", "slab_twice"):
        cuts = [c for c in p.plan[2] if c[1] > c[0]]
        lo, hi = cuts[-1] if what == "slab_missing" else cuts[0]
        acc += outer(lo, hi) * (-1.0 if what == "slab_missing" else 1.0)
    elif what == "n_chunk_clamped":
        c0 = (p.N - 1) & ~7
        acc[c0:] = A32[:m, c0 - 8:c0 - 8 + p.N - c0].t() @ B32[:m]
    elif what == "k_chunk_clamped":
        c0 = (p.K - 1) & ~7
        acc[:, c0:] = A32[:m].t() @ B32[:m, c0 - 8:c0 - 8 + p.K - c0]
    elif what == "transposed":
        acc = acc.t().clone()
    C = C0 + p.alpha * acc
    if what == "alpha_on_c0":
        C = p.alpha * (C0 + acc)
    elif what == "overwritten":
        C = p.alpha * acc
    buf = initial_buffer(p)
    buf[:p.N, :p.K] = C
    if what == "pad_column_written":
        buf[p.N - 1, p.K] = C[p.N - 1, p.K - 1]
    elif what == "row_N_written":
        buf[p.N, 0] = C[p.N - 1, 0]
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gemm_tn_edges_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
# a. row slicing of the 8-phase kernel: (M, splits, ns, rlast, ndup) -- the last three are what the launcher derives (asserted by the CPU test)
SLICING_TABLE = [
    (128, 1, 1, 128, 0),        # one pair of steps
    (256, 1, 1, 256, 0),
    (129, 1, 1, 128, 0),        # 1-row remainder pass
    (255, 1, 1, 128, 0),        # 127-row remainder pass
    (383, 1, 1, 256, 0),
    (257, 2, 2, 128, 127),      # TP_MASK(0) and TP_MASK(1)
    (319, 2, 2, 128, 65),
    (320, 2, 2, 128, 64),       # TP_MASK(0) only, exactly
    (321, 2, 2, 128, 63),
    (383, 2, 2, 128, 1),
    (384, 2, 2, 128, 0),
    (385, 3, 2, 256, 127),      # fewer slices than asked
    (640, 4, 3, 128, 0),        # a 128-row pair dropped
    (700, 3, 3, 256, 68),
    (300, 7, 3, 128, 84),       # splits far above the row blocks
    (1100, 5, 5, 128, 52),
    (1153, 4, 4, 128, 127),     # a pair dropped and the largest overlap
]
CASES_SLICING = [Problem(M, 256, 256, splits=s) for (M, s, *_) in SLICING_TABLE]

# b. column shapes of the 8-phase kernel: one 8-column tile; full tiles followed by an 8-column ragged tile, both ways; 3 tiles
COLUMN_SHAPES = [(8, 8), (264, 520), (520, 264), (136, 392), (768, 256)]
COLUMN_ROWS = [(255, 1), (320, 2), (1100, 5)]
CASES_COLUMNS = [Problem(M, N, K, splits=s, alpha=(1.0, -2.0)[(i + j) % 2])
                 for i, (N, K) in enumerate(COLUMN_SHAPES) for j, (M, s) in enumerate(COLUMN_ROWS)]

# c. device-side row count on the 8-phase kernel: the split route (re-cut on the device), the single-slice route, M < 256
COUNTS_SPLIT = [-3, 0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 384, 385, 512, 513, 640, 641, 700]
COUNT_SHAPES = [(256, 256), (264, 520)]
CASES_COUNT_SPLIT = [Problem(641, N, K, splits=4, count=c) for (N, K) in COUNT_SHAPES for c in COUNTS_SPLIT]
CASES_COUNT_SINGLE = [Problem(641, 256, 256, splits=1, count=c) for c in (0, 1, 640, 641)]
CASES_COUNT_SHORT = [Problem(200, 256, 256, splits=2, count=c, rows_buf=256) for c in (0, 100, 199, 200)]

# d. the 128x128 kernel: ragged last step, N % 8 == 4, grid.z slices (split counts that slice identically are listed once)
K1_ROWS = [1, 63, 64, 65, 127, 130, 1000]
K1_SHAPES = [(4, 4), (300, 132), (128, 128), (132, 260)]


def _k1_cases():
    seen, out = set(), []
    for M in K1_ROWS:
        for (N, K) in K1_SHAPES:
            for s in (1, 2, 3):
                p = Problem(M, N, K, splits=s, kernel=1)
                key = (M, N, K, tuple(p.plan[2]))
                if key not in seen:
                    seen.add(key)
                    out.append(p)
    return out


CASES_K1 = _k1_cases()
K1_COUNT_BASE = Problem(1000, 300, 132, splits=3, kernel=1)
CASES_K1_COUNT = [Problem(1000, 300, 132, splits=3, kernel=1, count=c) for c in (-1, 0, 1, 64, 333, 999, 1000, 1200)]

# e. the automatic choice either side of the tn_pick threshold: (shape, the forced kernel it must equal bit for bit)
CASES_AUTO = [((4096, 768, 768), 1), ((16384, 768, 768), 8)]

ALL_CASES = CASES_SLICING + CASES_COLUMNS + CASES_COUNT_SPLIT + CASES_COUNT_SINGLE + CASES_COUNT_SHORT + CASES_K1 + CASES_K1_COUNT


def case_id(p):
    return p.name
