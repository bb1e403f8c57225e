"""Host-side pieces of the k <= 1024 top-k: the ranking metrics of retrieval.py on a
hand-written example, and the three new entry points in the header and the binding."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def example():
    """Four queries over documents 0..999, 100 results each: the relevant document at rank 1,
    at rank 11, at rank 100, and absent."""
    top = torch.arange(100).repeat(4, 1) + 100 * torch.arange(4)[:, None]  # query i returns 100 i .. 100 i + 99
    relevant = [{0, 999}, {110}, {299, 998}, {5}]
    return top, relevant


def test_recall_at_k_and_mrr_at_k():
    from two_towers_amd.retrieval import mrr_at_k, recall_at_k
    top, relevant = example()
    assert recall_at_k(top, relevant) == {1: 0.25, 3: 0.25, 10: 0.25}
    assert recall_at_k(top, relevant, ks=(1, 10, 11, 99, 100)) == {1: 0.25, 10: 0.25, 11: 0.5, 99: 0.5, 100: 0.75}
    assert mrr_at_k(top, relevant) == pytest.approx((1.0 + 1.0 / 11 + 1.0 / 100 + 0.0) / 4, abs=1e-12)
    # a second relevant document further down changes neither: the first hit counts
    relevant[0].add(50)
    assert recall_at_k(top, relevant, ks=(1,)) == {1: 0.25}
    assert recall_at_k(top[:0], [], ks=(5,)) == {5: 0.0}


def test_header_and_binding_list_the_topk_entry_points():
    from two_towers_amd import _lib
    text = open(os.path.join(ROOT, "include", "tt_hip.h")).read()
    names = set(re.findall(r"^(?:int|long)\s+(tt_\w+)\(", text, re.M))
    for n in ("tt_topk_max", "tt_topk_rows", "tt_topk_rows_ws_size"):
        assert n in names and n in _lib.EXPORTED
    assert "min(16," not in text


def test_topk_limit_and_workspace_sizes():
    """tt_topk_max and the *_ws_size functions are host code. Up to k = 16 the sizes are
    what they were; above, they hold the rows x N fp32 score block."""
    from two_towers_amd import _lib
    lib = _lib.load()
    assert lib.tt_topk_max() == 1024 and _lib.topk_max() == 1024
    assert lib.tt_topk_rows_ws_size(100, 8192, 1024) == 0          # one chunk per row: no lists
    assert lib.tt_topk_rows_ws_size(4, 70000, 256) > 0
    assert lib.tt_topk_rows_ws_size(4, 70000, 1025) == 0           # invalid k: nothing to size
    Q, N, h = 8, 100000, 64
    small = lib.tt_search_ws_size(_lib.DT_BF16, Q, N, h, 16)
    large = lib.tt_search_ws_size(_lib.DT_BF16, Q, N, h, 17)
    assert small < Q * N * 4 <= large                              # Q <= 64, k <= 16: no score block
    assert lib.tt_hardneg_ws_size(_lib.DT_BF16, Q, N, 256, 16) < Q * N * 4 <= lib.tt_hardneg_ws_size(
        _lib.DT_BF16, Q, N, 256, 17)
