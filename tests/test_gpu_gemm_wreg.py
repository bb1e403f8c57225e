"""gemm_wreg, the B-resident short-K GEMM with the weights in registers (option bres_form 1:
each wave keeps a 64-column slice of B as MFMA fragments, the A rows stream through a
three-slot LDS ring by LDS-DMA), against the two kernels it must reproduce bit for bit on
the same operands: gemm_bres (bres_form 0, the panel of B in LDS) and the persistent
256 x 256 kernel (gemm_bres 0). Same MFMA instruction, operand roles and k order, one
rounding to bf16 after the fp32 bias: every output is identical as a bit pattern.

Shapes are the smallest at which each mechanism can fail (see the parametrisation). C is
prefilled with NaN and carries 64 sentinel rows after row M that no kernel may touch.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from two_towers_amd import ops  # noqa: E402

DEV = "cuda"
PANEL = 512  # gemm_wreg's column panel per workgroup (8 waves x 64 columns)
SENT = 64    # sentinel rows after row M


def rel_err(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


CASES = [
    # m, n, k, nbatch, bias, lda, new form expected
    # ragged last tile; of the 256 row groups 65 get one 64-row tile and the rest none: the
    # ring runs its prologue and drain with no steady state
    (4133, PANEL, 320, 1, True, 320, True),
    # the bench class: two batch entries, 16 row groups of 69 tiles, the last not full
    (70000, 3072, 320, 2, True, 320, True),
    # a single k-step (half a K-tile image), no bias
    (16384, 1536, 32, 1, False, 32, True),
    # a partial 64-deep image (K 96), A a column slice of a wider matrix (lda 160)
    (16421, PANEL, 96, 2, True, 160, True),
    # K 352 is outside the register budget (K <= 320): must run on gemm_bres and still match
    (40000, 384, 352, 2, True, 352, False),
]


@pytest.mark.parametrize("m,n,k,nb,with_bias,lda,wreg", CASES)
def test_gemm_weights_in_registers_matches_lds_panel_and_persistent(m, n, k, nb, with_bias, lda, wreg):
    from two_towers_amd import _lib
    from two_towers_amd._lib import option
    lib = _lib.load()
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    Aw = [torch.randn(m, lda, generator=g, device=DEV).to(dt) for _ in range(nb)]
    A = [a[:, :k] for a in Aw]
    B = [(torch.randn(n, k, generator=g, device=DEV) * k ** -0.5).to(dt) for _ in range(nb)]
    bias = [torch.randn(n, generator=g, device=DEV) for _ in range(nb)] if with_bias else None
    nan = torch.full((1,), float("nan"), dtype=dt).view(torch.int16).item()

    def run(form, bres):
        C = [torch.full((m + SENT, n), float("nan"), device=DEV, dtype=dt) for _ in range(nb)]
        with option("bres_form", form), option("gemm_bres", bres):
            which = lib.tt_gemm_bres_form(m, n, k, nb, lda, n)
            ops.gemm(Aw, B, C, m=m, n=n, k=k, lda=lda, ldb=k, ldc=n, a_kouter=False, b_kouter=False, dtype=dt,
                     out_dtype=dt, bias=bias, splits=1)
        torch.cuda.synchronize()
        for i in range(nb):
            tail = C[i][m:].view(torch.int16)
            assert int((tail != nan).sum()) == 0, f"form {form} bres {bres} batch {i}: sentinel rows written"
        return which, [c[:m] for c in C]

    which, new = run(1, 1)
    assert which == (2 if wreg else 1), which  # the weights-in-registers kernel really ran
    for form, bres in ((0, 1), (1, 0)):
        which, other = run(form, bres)
        assert which != 2 and (bres or which == 0), (form, bres, which)
        for i in range(nb):
            bad = int((new[i].view(torch.int16) != other[i].view(torch.int16)).sum())
            assert bad == 0, f"bres_form {form} gemm_bres {bres} batch {i}: {bad} of {m * n} outputs differ"
        del other
    # and against fp32 math on a sample of rows
    rows = torch.randint(0, m, (512,), generator=g, device=DEV)
    ref = A[0][rows].float() @ B[0].float().t() + (bias[0] if with_bias else 0)
    assert rel_err(new[0][rows].float(), ref) < 8e-3
