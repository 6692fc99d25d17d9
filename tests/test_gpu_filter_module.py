"""GPU: filtered retrieval at the public surface -- ``recommend*(where=...)`` on a small module with synthetic genres,
``ItemProcessor.search(where=...)`` against the hand-built exclusion list, cold-start items with tags, save / load."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_USERS, N_ITEMS, TOP = 30, 200, 10


def _module(mf, **cfg):
    m = mf.lightning.MatrixFactorizationLitModule({"num_users": N_USERS, "num_items": N_ITEMS, "hidden_size": 32, **cfg})
    m.configure_model(device=DEV)
    m.history = {3: [5, 6, 7, 8, 9, 10, 11, 12], 4: []}
    texts, _ = mf.data.synthetic_item_features(N_ITEMS, num_genres=6, seed=3)
    if cfg.get("item_tower") == "features":
        m.set_features(item=texts)
    m.on_validation_start()
    tags, vocab = mf.data.item_tag_bits(texts)
    m.set_item_tags(tags, vocab)
    return m, texts, tags, vocab


def _rows_with(tags, vocab, name):
    return set(np.flatnonzero((tags.numpy() >> vocab.index(name)) & 1).tolist())


@pytest.mark.parametrize("index_type", ["exact", "partitioned"])
def test_recommendations_carry_the_genre_and_keep_the_exclusions(mf, index_type):
    m, _, tags, vocab = _module(mf, index_type=index_type, num_partitions=4, num_probes=4)
    proc = m.item_processor
    assert torch.equal(proc.index.tags.cpu(), tags)
    for name in ("g0", "g3"):
        has = _rows_with(tags, vocab, name)
        where = {"any_of": [name]}
        rec = m.recommend_with_user_id(3, top_k=TOP, where=where)
        assert len(rec) == TOP and set(rec["movie_rn"]) <= has and not set(rec["movie_id"]) & set(m.history[3])
        assert rec.equals(m.recommend(3, top_k=TOP, where=proc.tag_filter(any_of=[name])))
        assert rec.equals(m.recommend_with_user_id(3, top_k=TOP, where=mf.retrieval.TagFilter(any_of=1 << vocab.index(name))))
        # ... and is the unfiltered search with every other item excluded by hand
        embed = m(torch.tensor([3], device=DEV)).detach().cpu().numpy()
        others = [i for i in range(N_ITEMS) if i not in has]
        want = proc.search(embed, exclude_item_ids=[*m.history[3], *others], top_k=TOP)
        assert rec.equals(want)
        item = sorted(has)[0]
        near = m.recommend_with_item_id(item, top_k=TOP, where=where)
        assert len(near) == TOP and set(near["movie_rn"]) <= has and item not in set(near["movie_id"])
        row = proc.index.embeddings[item: item + 1, :32].cpu().numpy()
        assert near.equals(proc.search(row, exclude_item_ids=[item, *others], top_k=TOP))
    none = m.recommend(4, top_k=TOP, where={"all_of": ["g0"], "none_of": ["g1"], "any_of": ["g2", "g3"]})
    ok = (_rows_with(tags, vocab, "g0") - _rows_with(tags, vocab, "g1")) & (_rows_with(tags, vocab, "g2") | _rows_with(tags, vocab, "g3"))
    assert set(none["movie_rn"]) <= ok and len(none) == min(TOP, len(ok))
    assert m.recommend(4, top_k=TOP).equals(m.recommend(4, top_k=TOP, where=None))
    with pytest.raises(KeyError, match="Western"):
        m.recommend(3, where={"any_of": ["Western"]})


def test_a_quantized_index_refuses_the_filter(mf):
    m, *_ = _module(mf, index_type="quantized", num_partitions=4, num_probes=4)
    with pytest.raises(NotImplementedError, match="QuantizedIndex"):
        m.recommend(3, top_k=TOP, where={"any_of": ["g0"]})
    assert len(m.recommend(3, top_k=TOP)) == TOP


def test_added_items_extend_the_tags_and_a_saved_module_keeps_them(mf, tmp_path):
    m, texts, tags, vocab = _module(mf, item_tower="features", feature_buckets=500)
    m.on_validation_start()                                            # (a new index: the tags stay, the row count matches)
    assert torch.equal(m.item_processor.index.tags.cpu(), tags)
    new = ['{"title":"Brand New (2031)","genres":["g0","g5"]}', '{"title":"Another (2032)","genres":["g1"]}']
    bits = torch.tensor([sum(1 << vocab.index(g) for g in json.loads(t)["genres"]) for t in new], dtype=torch.int64)
    m.add_items([9001, 9002], new, tags=bits)
    proc = m.item_processor
    assert proc.tags.numel() == N_ITEMS + 2 and torch.equal(proc.tags[-2:], bits) and torch.equal(proc.index.tags.cpu(), proc.tags)
    both = proc.tag_filter(all_of=["g0", "g5"])
    rec = m.recommend_with_item_id(9001, top_k=N_ITEMS, where=both)
    want = set(np.flatnonzero((proc.tags.numpy() & both.all_of) == both.all_of).tolist()) - {N_ITEMS}
    assert set(rec["movie_rn"]) == want and 9001 not in set(rec["movie_id"])
    assert N_ITEMS in set(m.recommend(3, top_k=N_ITEMS + 2, where=both)["movie_rn"])
    m.add_items([9003], ['{"title":"Untagged (2033)","genres":["g2"]}'])
    assert int(proc.tags[-1]) == 0 and proc.index.tags.numel() == N_ITEMS + 3
    with pytest.raises(ValueError, match="one int64 word per new item"):
        m.add_items([9004], ['{"title":"x","genres":[]}'], tags=torch.zeros(2, dtype=torch.int64))

    m.save(tmp_path / "model")
    m2 = mf.lightning.MatrixFactorizationLitModule.load(tmp_path / "model", device=DEV)
    assert m2.item_processor.tag_vocabulary == vocab and torch.equal(m2.item_processor.tags, proc.tags)
    assert torch.equal(m2.item_processor.index.tags.cpu(), proc.tags)
    for where in ({"any_of": ["g0"]}, {"all_of": ["g0", "g5"]}, {"none_of": ["g0", "g1", "g2"]}):
        assert m2.recommend(3, top_k=TOP, where=where).equals(m.recommend(3, top_k=TOP, where=where))
        assert m2.recommend_with_item_id(9001, top_k=TOP, where=where).equals(m.recommend_with_item_id(9001, top_k=TOP, where=where))
