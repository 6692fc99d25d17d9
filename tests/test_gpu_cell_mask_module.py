"""GPU: ``filter_mode="mask"`` at the public surface -- ``recommend*(where=...)`` on a small module whose partitioned or quantised
index filters in place (``search(allow=...)``), against the processor's search with the hand-built exclusion list; the default
``filter_mode="view"`` on a quantised index still refuses."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_USERS, N_ITEMS, TOP = 30, 200, 10


def _module(mf, **cfg):
    m = mf.lightning.MatrixFactorizationLitModule({"num_users": N_USERS, "num_items": N_ITEMS, "hidden_size": 32, "num_partitions": 4,
                                                   "num_probes": 4, **cfg})
    m.configure_model(device=DEV)
    m.history = {3: [5, 6, 7, 8, 9, 10, 11, 12], 4: []}
    texts, _ = mf.data.synthetic_item_features(N_ITEMS, num_genres=6, seed=3)
    m.on_validation_start()
    tags, vocab = mf.data.item_tag_bits(texts)
    m.set_item_tags(tags, vocab)
    return m, tags, vocab


def _rows_with(tags, vocab, name):
    return set(np.flatnonzero((tags.numpy() >> vocab.index(name)) & 1).tolist())


@pytest.mark.parametrize("index_type", ["partitioned", "quantized"])
def test_recommendations_through_the_mask_equal_the_hand_built_exclusion(mf, index_type):
    m, tags, vocab = _module(mf, index_type=index_type, filter_mode="mask")
    proc = m.item_processor
    assert proc.filter_mode == "mask" and type(proc.index).__name__ == {"partitioned": "PartitionedIndex", "quantized": "QuantizedIndex"}[index_type]
    for name in ("g0", "g3"):
        has = _rows_with(tags, vocab, name)
        assert 0 < len(has) < N_ITEMS
        where = {"any_of": [name]}
        rec = m.recommend_with_user_id(3, top_k=TOP, where=where)
        assert len(rec) == TOP and set(rec["movie_rn"]) <= has and not set(rec["movie_id"]) & set(m.history[3])
        assert rec.equals(m.recommend(3, top_k=TOP, where=proc.tag_filter(any_of=[name])))
        embed = m(torch.tensor([3], device=DEV)).detach().cpu().numpy()
        others = [i for i in range(N_ITEMS) if i not in has]
        assert rec.equals(proc.search(embed, exclude_item_ids=[*m.history[3], *others], top_k=TOP))
        assert not rec.equals(m.recommend(3, top_k=TOP))
        item = sorted(has)[0]
        near = m.recommend_with_item_id(item, top_k=TOP, where=where)
        assert len(near) == TOP and set(near["movie_rn"]) <= has and item not in set(near["movie_id"])
        row = proc.index.embeddings[item: item + 1, :32].cpu().numpy()
        assert near.equals(proc.search(row, exclude_item_ids=[item, *others], top_k=TOP))
    assert len(proc.index._masks) == 2 and len(proc.index._views) == 0              # a mask per filter, and no copy of rows
    allow = torch.from_numpy(((tags.numpy() >> vocab.index("g1")) & 1).astype(bool))
    assert m.recommend(4, top_k=TOP, where=allow).equals(m.recommend(4, top_k=TOP, where={"any_of": ["g1"]}))
    assert m.recommend(4, top_k=TOP).equals(m.recommend(4, top_k=TOP, where=None))


def test_the_default_mode_keeps_its_behaviour(mf):
    m, tags, vocab = _module(mf, index_type="quantized")
    assert m.item_processor.filter_mode == "view"
    with pytest.raises(NotImplementedError, match="QuantizedIndex"):
        m.recommend(3, top_k=TOP, where={"any_of": ["g0"]})
    assert len(m.recommend(3, top_k=TOP)) == TOP
    view, _, _ = _module(mf, index_type="partitioned")
    mask, _, _ = _module(mf, index_type="partitioned", filter_mode="mask")
    mask.towers.load_state_dict(view.towers.state_dict())
    mask.on_validation_start()
    mask.set_item_tags(tags, vocab)
    for where in ({"any_of": ["g0"]}, {"all_of": ["g0"], "none_of": ["g1"]}):
        assert mask.recommend(3, top_k=TOP, where=where).equals(view.recommend(3, top_k=TOP, where=where))
    assert len(view.item_processor.index._views) == 2 and len(view.item_processor.index._masks) == 0
