"""Host side of the trainable embedding table: the EmbeddingTable module, how the models
take it, and the (perm, seg_ptr, unique) plan of tt_embed_grad_rows. No GPU needed."""
import numpy as np
import pytest
import torch

import two_towers_amd as tta
from two_towers_amd import ops
from two_towers_amd.embedding import EmbeddingTable, table_of
from two_towers_amd.margin import TwoTowerModel


def test_embedding_table_construction():
    w = torch.randn(7, 5, dtype=torch.float64)
    t = tta.EmbeddingTable(w)
    assert isinstance(t.weight, torch.nn.Parameter) and t.weight.dtype == torch.float32
    assert tuple(t.weight.shape) == (7, 5) and t.weight.requires_grad and t.trainable
    assert t.num_embeddings == 7 and t.embedding_dim == 5
    assert torch.equal(t.weight.detach(), w.float())
    w[0, 0] += 1  # a copy, not a view of the source
    assert not torch.equal(t.weight.detach(), w.float())
    f = tta.EmbeddingTable(w, trainable=False)
    assert not f.weight.requires_grad and not f.trainable
    assert list(t.state_dict()) == ["weight"]
    f.load_state_dict(t.state_dict())
    assert torch.equal(f.weight, t.weight)
    assert table_of(t.weight) is t and table_of(f.weight) is f and table_of(torch.nn.Parameter(w)) is None


def test_embedding_table_from_vocab_and_array():
    vec = np.arange(12, dtype=np.float32).reshape(4, 3)
    v = tta.Vocab(["a", "b", "c", "d"], vec)
    for src in (v, vec):
        t = tta.EmbeddingTable(src)
        assert torch.equal(t.weight.detach(), torch.from_numpy(vec))


@pytest.mark.parametrize("bad", [torch.randn(5), torch.randn(2, 3, 4), torch.zeros(3, 4, dtype=torch.int64),
                                 torch.zeros(0, 4), "words"])
def test_embedding_table_validation(bad):
    with pytest.raises((ValueError, TypeError)):
        tta.EmbeddingTable(bad)


def models(E=6, h=8):
    return [tta.EnhancedTwoTowerModel(E, h), TwoTowerModel(E, h), tta.SimpleTwoTower(E, h)]


def test_set_embedding_table_accepts_module_or_tensor():
    for m in models():
        assert m.set_embedding_table(torch.randn(9, 6)) is m
        assert isinstance(m._table_src, torch.Tensor)
        t = tta.EmbeddingTable(torch.randn(9, 6))
        assert m.set_embedding_table(t) is m
        assert m._table_src is t
        with pytest.raises(ValueError):
            m.set_embedding_table(tta.EmbeddingTable(torch.randn(9, 5)))
        with pytest.raises(ValueError):
            m.set_embedding_table(torch.randn(9, 5))
        m.set_embedding_table(None)
        assert m._table_src is None


def test_state_dict_keys_unchanged_with_table_module():
    for m in models():
        before = list(m.state_dict())
        nparam = len(list(m.parameters()))
        m.set_embedding_table(tta.EmbeddingTable(torch.randn(9, 6)))
        assert list(m.state_dict()) == before
        assert len(list(m.parameters())) == nparam
        assert not any(isinstance(s, EmbeddingTable) for s in m.modules())
    assert len(tta.EnhancedTwoTowerModel(6, 8).state_dict()) == 44


def plain_plan(ids):
    """Positions of each id >= 0 in order of appearance, ids ascending."""
    groups = {}
    for pos, i in enumerate(ids):
        if i >= 0:
            groups.setdefault(i, []).append(pos)
    uniq = sorted(groups)
    perm = [p for u in uniq for p in groups[u]]
    seg = [0]
    for u in uniq:
        seg.append(seg[-1] + len(groups[u]))
    return perm, seg, uniq


@pytest.mark.parametrize("case", ["mixed", "all_pad", "single_id", "one", "distinct", "empty"])
def test_embed_plan_matches_plain_grouping(case):
    g = torch.Generator().manual_seed(3)
    ids = {
        "mixed": torch.randint(-1, 12, (5, 9), generator=g),
        "all_pad": torch.full((3, 4), -1),
        "single_id": torch.full((2, 7), 4),
        "one": torch.tensor([[6]]),
        "distinct": torch.randperm(20, generator=g).reshape(4, 5),
        "empty": torch.zeros(0, 3, dtype=torch.int64),
    }[case]
    for dt in (torch.int32, torch.int64):
        perm, seg_ptr, uniq = ops.embed_plan(ids.to(dt))
        rp, rs, ru = plain_plan(ids.reshape(-1).tolist())
        assert perm.dtype == torch.int32 and seg_ptr.dtype == torch.int32 and uniq.dtype == torch.int64
        assert perm.tolist() == rp and seg_ptr.tolist() == rs and uniq.tolist() == ru


def test_sparse_adam_rejects_bad_hyperparameters():
    p = torch.nn.Parameter(torch.zeros(3, 2))
    with pytest.raises(ValueError):
        tta.SparseAdam([p], lr=-1.0)
    with pytest.raises(ValueError):
        tta.SparseAdam([p], betas=(1.0, 0.9))
    assert tta.optim.SparseAdam is tta.SparseAdam
