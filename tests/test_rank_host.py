"""Host-side pieces of the full-rank evaluation (validate_margin.py:11-54 without a top-k
cutoff): the CSR form of the relevance sets, the metrics derived from ranks, the error for
CPU tensors, and the entry points in the header, the binding and the option table."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relevance_csr_empty_rows_duplicates_and_unsorted_input():
    from two_towers_amd import relevance_csr
    ptr, idx = relevance_csr([{5, 2}, [], (9, 9, 1, 9), [7], set(), iter([3, 0, 3])])
    assert ptr.dtype == torch.int32 and idx.dtype == torch.int32
    assert ptr.tolist() == [0, 2, 2, 4, 5, 5, 7]
    assert idx.tolist() == [2, 5, 1, 9, 7, 0, 3]
    ptr, idx = relevance_csr([])
    assert ptr.tolist() == [0] and idx.tolist() == [] and idx.dtype == torch.int32
    ptr, idx = relevance_csr([[], []])
    assert ptr.tolist() == [0, 0, 0] and idx.numel() == 0


def test_mrr_from_ranks_counts_rank_zero_as_a_miss():
    from two_towers_amd import mrr_from_ranks
    assert mrr_from_ranks(torch.tensor([1, 11, 100, 0], dtype=torch.int32)) == pytest.approx(
        (1.0 + 1.0 / 11 + 1.0 / 100 + 0.0) / 4, abs=1e-12)
    assert mrr_from_ranks([0, 0]) == 0.0
    assert mrr_from_ranks([2]) == 0.5
    assert mrr_from_ranks(torch.zeros(0, dtype=torch.int32)) == 0.0
    # a rank far past any top-k still counts: that is the point of the full rank
    assert mrr_from_ranks([1000000]) == pytest.approx(1e-6, rel=1e-12)


def test_recall_from_ranks():
    from two_towers_amd import recall_from_ranks
    ranks = torch.tensor([1, 11, 100, 0, 3], dtype=torch.int32)
    assert recall_from_ranks(ranks) == {1: 0.2, 3: 0.4, 10: 0.4}
    assert recall_from_ranks(ranks, ks=(11, 99, 100, 5000)) == {11: 0.6, 99: 0.6, 100: 0.8, 5000: 0.8}
    assert recall_from_ranks(torch.zeros(0, dtype=torch.int32), ks=(5,)) == {5: 0.0}
    assert recall_from_ranks([0, 0], ks=(1,)) == {1: 0.0}


def test_first_relevant_rank_refuses_cpu_tensors():
    from two_towers_amd import _lib, first_relevant_rank
    q, d = torch.randn(3, 16), torch.randn(5, 16)
    with pytest.raises(_lib.TTError, match="only on an AMD GPU"):
        first_relevant_rank(q, d, [{0}, {1}, set()])


def test_header_binding_and_option_list_the_rank_entry_points():
    from two_towers_amd import _lib
    text = open(os.path.join(ROOT, "include", "tt_hip.h")).read()
    names = set(re.findall(r"^(?:int|long)\s+(tt_\w+)\(", text, re.M))
    lib = _lib.load()
    for n in ("tt_rank_best_relevant", "tt_rank_count", "tt_rank_count_ws_size"):
        assert n in names and n in _lib.EXPORTED and hasattr(lib, n)
    assert _lib.get_option("rank_gemm") == 0


def test_rank_count_workspace_and_argument_checks():
    """Host code only: the fused shapes need no score block, the stored path at most 1 GiB of
    it, and bad arguments are refused before anything is launched."""
    from two_towers_amd import _lib
    lib = _lib.load()
    Q, N = 8192, 65536
    assert lib.tt_rank_count_ws_size(_lib.DT_BF16, Q, N, 256) < Q * 4
    stored = lib.tt_rank_count_ws_size(_lib.DT_F32, Q, N, 256)
    assert N * 4 <= stored <= 1 << 30
    assert lib.tt_rank_count_ws_size(_lib.DT_BF16, 100, 1000, 96) == 100 * 1000 * 4 + (-(100 * 1000 * 4)) % 256
    old = _lib.get_option("rank_gemm")
    try:
        lib.tt_set_option(b"rank_gemm", 1)
        assert lib.tt_rank_count_ws_size(_lib.DT_BF16, Q, N, 256) == stored
    finally:
        lib.tt_set_option(b"rank_gemm", old)
    # Q = 0 is a no-op; h must be a multiple of 8; misaligned rows are refused
    assert lib.tt_rank_count(_lib.DT_BF16, None, 0, None, 10, 256, 0, None, None, None, 0, None, None) == 0
    assert lib.tt_rank_best_relevant(_lib.DT_F32, None, 0, None, 10, 64, None, None, None, None, None, None) == 0
    assert lib.tt_rank_count(_lib.DT_F32, 16, 4, 16, 10, 12, 0, 16, 16, 16, 0, 16, None) == 1000
    assert lib.tt_rank_count(_lib.DT_BF16, 18, 4, 16, 10, 256, 0, 16, 16, 16, 0, 16, None) == 1000
    assert b"aligned" in lib.tt_last_error()
    assert lib.tt_rank_count(_lib.DT_BF16, 16, 4, 16, 10, 256, -1, 16, 16, 16, 0, 16, None) == 1000
