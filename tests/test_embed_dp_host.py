"""dist.union_of, the index plumbing of a data-parallel trainable table: the ascending union of
the ranks' distinct ids and each rank's positions inside it, against numpy.union1d /
searchsorted. No GPU and no process group needed."""
import numpy as np
import pytest
import torch

from two_towers_amd import dist

CASES = {
    "partial_overlap": [[1, 4, 9, 30], [0, 4, 5, 30, 199], [9, 10, 11]],
    "one_empty": [[3, 7], [], [2, 3, 100]],
    "all_empty": [[], [], []],
    "identical": [[5, 6, 8], [5, 6, 8]],
    "single": [[0, 2, 2 ** 31 + 5]],
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_union_of_matches_numpy(case):
    lists = [torch.tensor(x, dtype=torch.int64) for x in CASES[case]]
    guniq, dsts = dist.union_of(lists)
    ref = np.array([], dtype=np.int64)
    for x in CASES[case]:
        ref = np.union1d(ref, np.array(x, dtype=np.int64))
    assert guniq.dtype == torch.int64 and guniq.dim() == 1
    assert np.array_equal(guniq.numpy(), ref)
    g = guniq.numpy()
    assert bool((np.diff(g) > 0).all())  # ascending and distinct
    assert len(dsts) == len(lists)
    for ids, dst in zip(lists, dsts):
        assert dst.dtype == torch.int32 and tuple(dst.shape) == tuple(ids.shape)
        assert np.array_equal(dst.numpy(), np.searchsorted(ref, ids.numpy()))
        assert torch.equal(guniq[dst.long()], ids)
        assert bool((np.diff(dst.numpy()) > 0).all())  # strictly ascending: tt_embed_grad_rows_at's contract


def test_union_ids_without_a_process_group_is_the_identity():
    ids = torch.tensor([2, 5, 11], dtype=torch.int64)
    guniq, dst = dist.union_ids(ids, None)
    assert torch.equal(guniq, ids) and dst.dtype == torch.int32 and dst.tolist() == [0, 1, 2]
