"""Host-side pieces of the int8 document index: the entry points in the header, the binding
and the built library, the workspace size, and the errors raised before anything is launched."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tt_quantize_rows_i8", "tt_search_topk_i8", "tt_search_i8_ws_size", "tt_gather_scores")


def test_header_binding_and_library_list_the_int8_entry_points():
    from two_towers_amd import _lib
    text = open(os.path.join(ROOT, "include", "tt_hip.h")).read()
    names = set(re.findall(r"^(?:int|long)\s+(tt_\w+)\(", text, re.M))
    lib = _lib.load()
    for n in NAMES:
        assert n in names and n in _lib.EXPORTED and hasattr(lib, n), n
    assert _lib.get_option("search_i8_qb") == 0
    assert "2^24" in text and "h <= 1024" in text  # the reason for the cap is stated


def test_workspace_size_positive_and_monotone_in_q():
    from two_towers_amd import _lib
    lib = _lib.load()
    qs = (1, 2, 8, 63, 64, 65, 66, 100, 128, 255, 256, 257, 1000, 4096, 20000)
    for N, h, k in ((100000, 512, 3), (100000, 64, 16), (5000, 128, 100), (1 << 21, 512, 1024), (17, 16, 1)):
        sizes = [lib.tt_search_i8_ws_size(Q, N, h, k) for Q in qs]
        assert all(s > 0 for s in sizes), (N, h, k, sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (N, h, k, sizes)
        if k > 16 or qs[-1] > 64:
            assert sizes[-1] >= qs[-1] * N * 4  # a stored score block
    # the fused scan keeps no score block: candidates only
    assert lib.tt_search_i8_ws_size(1, 1 << 21, 512, 3) < (1 << 21)
    assert lib.tt_search_i8_ws_size(2, 1 << 21, 512, 16) < 2 * (1 << 21) * 4


def test_bad_arguments_are_refused_before_any_launch():
    from two_towers_amd import _lib
    lib = _lib.load()
    assert lib.tt_search_topk_i8(None, None, 0, None, None, 10, 64, 3, None, None, None, None) == 0  # Q = 0
    assert lib.tt_quantize_rows_i8(None, 0, 64, 64, None, None, None) == 0  # rows = 0
    assert lib.tt_search_topk_i8(16, 16, 2, 16, 16, 10, 24, 3, 16, 16, 16, None) == _lib.TT_EINVAL
    assert b"multiple of 16" in lib.tt_last_error()
    assert lib.tt_search_topk_i8(16, 16, 2, 16, 16, 10, 1040, 3, 16, 16, 16, None) == _lib.TT_EINVAL
    assert b"at most 1024" in lib.tt_last_error()
    assert lib.tt_search_topk_i8(16, 16, 2, 16, 16, 10, 64, 11, 16, 16, 16, None) == _lib.TT_EINVAL
    assert b"min(1024, N=10)" in lib.tt_last_error()
    assert lib.tt_search_topk_i8(16, 16, 2, 16, 16, 5000, 64, 1025, 16, 16, 16, None) == _lib.TT_EINVAL
    assert lib.tt_search_topk_i8(16, 16, 2, 17, 16, 10, 64, 3, 16, 16, 16, None) == _lib.TT_EINVAL
    assert b"aligned" in lib.tt_last_error()
    assert lib.tt_quantize_rows_i8(16, 4, 24, 24, 16, 16, None) == _lib.TT_EINVAL
    assert lib.tt_quantize_rows_i8(16, 4, 64, 66, 16, 16, None) == _lib.TT_EINVAL  # ld % 4
    assert lib.tt_gather_scores(_lib.DT_F32, 16, 2, 16, 10, 60, 16, 4, 16, None) == _lib.TT_EINVAL
    assert lib.tt_gather_scores(_lib.DT_F32, 16, 2, 16, 10, 64, 16, 1025, 16, None) == _lib.TT_EINVAL
    assert lib.tt_gather_scores(7, 16, 2, 16, 10, 64, 16, 4, 16, None) == _lib.TT_EINVAL


def test_cpu_tensors_are_refused_with_the_projects_error():
    from two_towers_amd import _lib, ops
    from two_towers_amd.retrieval import topk_cosine
    from two_towers_amd.serving import SearchIndex
    with pytest.raises(_lib.TTError, match="only on an AMD GPU"):
        ops.quantize_rows_i8(torch.randn(4, 64))
    with pytest.raises(_lib.TTError, match="only on an AMD GPU"):
        ops.gather_scores(torch.randn(2, 64), torch.randn(9, 64), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(_lib.TTError, match="only on an AMD GPU"):
        topk_cosine(torch.randn(2, 64), torch.randn(9, 64), k=3, compute_dtype=torch.int8)
    with pytest.raises(_lib.TTError, match="only on an AMD GPU"):
        SearchIndex(object(), None, ["a", "b", "c"], doc_vectors=torch.randn(3, 64), device="cpu",
                    score_dtype=torch.int8)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_rescore_needs_the_int8_index(dt):
    from two_towers_amd.serving import SearchIndex
    with pytest.raises(ValueError, match="rescore"):
        SearchIndex(object(), None, ["a", "b", "c"], doc_vectors=torch.randn(3, 64), device="cpu",
                    score_dtype=dt, rescore=4)
    with pytest.raises(ValueError, match="score_dtype"):
        SearchIndex(object(), None, ["a", "b", "c"], doc_vectors=torch.randn(3, 64), device="cpu",
                    score_dtype=torch.float16)
