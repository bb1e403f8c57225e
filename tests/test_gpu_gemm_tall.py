"""gemm_tall (option wgrad_tall 1; 2 and 3 force its whole-tile and half-tile forms): one
320-row tile per 256-column panel for bf16 TN products with 256 < M <= 320, the layer-0
dW_ih^T = X0^T dG shape, against the kernel it
replaces (option 0: gemm_kernel's 256-row tile plus a tail tile) at the same forced split
count. Both accumulate every output in the same ascending 32-deep MFMA steps with the same
split boundaries and reduce the slices in the same order, so the outputs are equal bit for
bit; the new form is also checked against float64 math at the bound
test_gemm_tail_tile_idle_wave_row uses.

C and the split-K workspace are prefilled with NaN; C carries sentinel rows after row M and
sentinel columns after column N that no kernel may touch. Operand columns past M (A) and
past N (B) inside the leading dimension hold NaN: they must not reach any output.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from two_towers_amd import _lib, ops  # noqa: E402
from two_towers_amd._lib import GemmBatch, option  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
SENT_R, SENT_C = 16, 8  # sentinel rows after M, columns after N
X_BIAS, X_RELU, X_DROP, X_SHIFT, X_ASPLIT, X_ACC = 1, 2, 4, 8, 16, 32  # tt_gemm_tall_form extras


def rel_err(a, b):
    a = a.double()
    b = b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def form(m, n, k, lda, ldb, splits, dtype=BF, extras=0):
    code = _lib.dtype_code(dtype)
    return _lib.load().tt_gemm_tall_form(code, _lib.DT_F32, 1, 1, m, n, k, lda, ldb, splits, extras)


def gemm_tn(A, B, m, n, k, lda, ldb, splits, c_trans=False):
    """tt_gemm_ct on K-outer bf16 operands with fp32 out; returns the padded, NaN-prefilled C
    buffers ([m + SENT_R, n + SENT_C], or [n + SENT_R, m + SENT_C] for c_trans)."""
    lib = _lib.load()
    nb = len(A)
    rows, cols = (n, m) if c_trans else (m, n)
    C = [torch.full((rows + SENT_R, cols + SENT_C), float("nan"), device=DEV) for _ in range(nb)]
    bt = GemmBatch()
    for i in range(nb):
        bt.a[i], bt.b[i], bt.c[i] = A[i].data_ptr(), B[i].data_ptr(), C[i].data_ptr()
    nws = lib.tt_gemm_ws_size(m, n, nb, splits)
    ws = torch.full((max(nws, 1),), float("nan"), device=DEV)
    _lib.call("tt_gemm_ct", _lib.DT_BF16, _lib.DT_F32, 1, 1, m, n, k, ctypes.byref(bt), nb, lda, ldb, cols + SENT_C,
              1.0, 0, 0, 0, 0, 0.0, splits, ws.data_ptr() if nws else None, int(c_trans), _lib.stream_ptr(C[0].device))
    torch.cuda.synchronize()
    return C


def check_untouched(C, rows, cols, what):
    for i, c in enumerate(C):
        assert bool(torch.isnan(c[rows:]).all()), f"{what} batch {i}: sentinel rows written"
        assert bool(torch.isnan(c[:, cols:]).all()), f"{what} batch {i}: sentinel columns written"
        assert not bool(torch.isnan(c[:rows, :cols]).any()), f"{what} batch {i}: NaN in the output"


def operands(m, n, k, lda, ldb, nb, seed):
    """K-outer A [k, lda] and B [k, ldb] with NaN in the columns past m / n."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    A, B = [], []
    for _ in range(nb):
        a = torch.randn(k, lda, generator=g, device=DEV).to(BF)
        b = torch.randn(k, ldb, generator=g, device=DEV).to(BF)
        a[:, m:] = float("nan")
        b[:, n:] = float("nan")
        A.append(a)
        B.append(b)
    return A, B


def compare(A, B, m, n, k, lda, ldb, splits):
    """New form against the old at equal splits (bit-identical) and against float64."""
    with option("wgrad_tall", 0):
        assert form(m, n, k, lda, ldb, splits) == 0
        old = gemm_tn(A, B, m, n, k, lda, ldb, splits)
    check_untouched(old, m, n, "wgrad_tall 0")
    refs = [A[i][:, :m].double().t() @ B[i][:, :n].double() for i in range(len(A))]
    # 1: the default (whole tiles, a thin last round as half tiles), 2: whole 320-row tiles
    # only, 3: half tiles only (two workgroups of 160 rows per tile)
    for mode in (1, 2, 3):
        with option("wgrad_tall", mode):
            assert form(m, n, k, lda, ldb, splits) == 1, "gemm_tall expected for this shape"
            new = gemm_tn(A, B, m, n, k, lda, ldb, splits)
        check_untouched(new, m, n, f"wgrad_tall {mode}")
        for i in range(len(A)):
            assert torch.equal(new[i][:m, :n], old[i][:m, :n]), \
                f"mode {mode} batch {i}: {int((new[i][:m, :n] != old[i][:m, :n]).sum())} of {m * n} outputs differ"
            e = rel_err(new[i][:m, :n], refs[i])
            print(f"mode {mode} m {m} n {n} k {k} splits {splits} batch {i}: rel_err {e:.3e}")
            assert e < 1e-5, e


CASES = [
    # m, n, k, lda, ldb, splits
    (320, 1536, 8192, 320, 1536, 1),   # the step's tile, six column panels, no split
    (320, 1536, 8192, 320, 1536, 3),   # 128 K-tiles in slices of 43, 43, 42: a ragged last slice
    (264, 256, 1024, 320, 256, 1),     # M tail inside the narrow sub-image: 8 of its 64 columns live
    (304, 256, 1024, 304, 256, 2),     # 48 of 64 live, lda = M: the operand ends where the tile's rows do
    (320, 200, 1024, 320, 256, 1),     # ragged column panel ending on a whole 16-byte chunk
    (320, 256, 64, 320, 256, 1),       # one K-tile: the ring's prologue and drain only
    (320, 256, 8200, 320, 256, 1),     # K tail of 8 rows: the last K-tile reads zeros past K
    (320, 256, 8200, 320, 256, 3),     # ... and as the ragged last slice of a split
    # 6 panels x 44 one-K-tile slices = 264 tiles: the default runs 256 whole and 8 as halves
    (320, 1536, 2816, 320, 1536, 44),
]


@pytest.mark.parametrize("m,n,k,lda,ldb,splits", CASES)
def test_tall_tile_matches_padded_tiles_bitwise(m, n, k, lda, ldb, splits):
    A, B = operands(m, n, k, lda, ldb, 1, m + n + k + splits)
    compare(A, B, m, n, k, lda, ldb, splits)


def test_tall_tile_four_problems_with_step_strides():
    """The step's call: (tower, direction) problems, A = X0 [K, 320], B = the 1536-column gate
    blocks at columns 0 and 1536 of a tower's [K, 4096] gate-gradient buffer."""
    m, n, k = 320, 1536, 2048
    g = torch.Generator(device=DEV).manual_seed(5)
    X0 = [torch.randn(k, m, generator=g, device=DEV).to(BF) for _ in range(2)]
    dG = [torch.randn(k, 4096, generator=g, device=DEV).to(BF) for _ in range(2)]
    for d in dG:
        d[:, 2 * n:] = float("nan")  # the columns after the two gate blocks are not operands
    A = [X0[i // 2] for i in range(4)]
    B = [dG[i // 2][:, (i % 2) * n:] for i in range(4)]
    compare(A, B, m, n, k, m, 4096, 3)


def test_reduction_writes_transposed_output():
    """tt_gemm_ct's c_trans: the split-K reduction writes C as [n][m] with the sums of the
    plain call, for the new form and the old."""
    m, n, k, splits = 320, 1536, 2048, 3
    A, B = operands(m, n, k, m, n, 2, 11)
    for tall in (1, 0):
        with option("wgrad_tall", tall):
            assert form(m, n, k, m, n, splits) == tall
            assert _lib.load().tt_gemm_pick_splits(m, n, 524288, 4) == 16  # the split count does not move
            c = gemm_tn(A, B, m, n, k, m, n, splits)
            ct = gemm_tn(A, B, m, n, k, m, n, splits, c_trans=True)
        check_untouched(c, m, n, f"wgrad_tall {tall}")
        check_untouched(ct, n, m, f"wgrad_tall {tall} c_trans")
        for i in range(2):
            assert torch.equal(ct[i][:n, :m], c[i][:m, :n].t()), (tall, i)
    with pytest.raises(RuntimeError):  # nothing transposes a one-split call
        gemm_tn(A, B, m, n, k, m, n, 1, c_trans=True)


def test_other_shapes_keep_the_general_kernels():
    with option("wgrad_tall", 1):
        assert form(320, 1536, 8192, 320, 1536, 1) == 1
        assert form(320, 1536, 8192, 320, 1536, 16) == 1
        assert form(256, 1536, 8192, 256, 1536, 1) == 0
        assert form(328, 1536, 8192, 328, 1536, 1) == 0
        assert form(316, 1536, 8192, 320, 1536, 1) == 0  # M not in whole 16-byte chunks
        assert form(320, 1536, 8192, 320, 1536, 1, dtype=torch.float32) == 0
        assert form(320, 1536, 8192, 320, 1536, 1, extras=X_BIAS) == 0
        assert form(320, 1536, 8192, 320, 1536, 1, extras=X_ASPLIT) == 0
        for x in (X_RELU, X_DROP, X_SHIFT, X_ACC):
            assert form(320, 1536, 8192, 320, 1536, 1, extras=x) == 0
    with option("wgrad_tall", 0):
        assert form(320, 1536, 8192, 320, 1536, 1) == 0


def test_calls_with_bias_or_a_split_run_the_general_kernels():
    """A biased call and an a_split call of the tall shape through ops.gemm with the option on:
    served by the general kernels, against float64."""
    m, n, k = 320, 256, 1024
    A, B = operands(m, n, k, m, n, 1, 23)
    bias = torch.randn(n, device=DEV)
    ref = A[0].double().t() @ B[0].double()
    with option("wgrad_tall", 1):
        C = torch.full((m, n), float("nan"), device=DEV)
        ops.gemm(A, B, [C], m=m, n=n, k=k, lda=m, ldb=n, ldc=n, a_kouter=True, b_kouter=True, dtype=BF,
                 out_dtype=torch.float32, bias=[bias], splits=1)
        assert rel_err(C, ref + bias.double()) < 1e-5
        hi = A[0][:, 256:].contiguous()  # columns >= 256 from a second buffer (same lda needed)
        hi_w = torch.zeros(k, m, device=DEV, dtype=BF)
        hi_w[:, :64] = hi
        C2 = torch.full((m, n), float("nan"), device=DEV)
        ops.gemm(A, B, [C2], m=m, n=n, k=k, lda=m, ldb=n, ldc=n, a_kouter=True, b_kouter=True, dtype=BF,
                 out_dtype=torch.float32, a_hi=[hi_w], a_split=256, splits=1)
        assert rel_err(C2, ref) < 1e-5
