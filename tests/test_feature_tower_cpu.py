"""CPU: the spec of the hashed feature-bag towers (``spec_bag``, plain torch -- the GPU tests hold the kernels to it), the
tokenizer, the MovieLens attribute readers, the configuration surface and the new kernels' register budgets.

Spec.  A bag is a list of (token t_e, weight w_e); the feature table F is [R, d].  Tokens outside [1, R) are padding and
are dropped everywhere (sums, weight sums, counts).  Weights are finite and >= 0 (1 when none are given).
s_b = sum_valid w_e F[t_e] (rows not normalised, as torch.nn.EmbeddingBag); p_b = s_b ("sum"), s_b / sum w_e ("mean"),
s_b / sqrt(sum w_e^2) ("sqrtn"); an empty bag or a zero weight sum gives p_b = 0 and no gradient;
u_b = normalize ? p_b / max(|p_b|, 1e-12) : p_b.  dL/dF[t] = sum_{e: t_e = t} w_e c_b g_p,b with c_b the combiner factor."""
from __future__ import annotations

import hashlib
import importlib.util
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests.conftest import ROOT


def spec_bag(w: torch.Tensor, lists, weights=None, combiner: str = "mean", normalize: bool = True) -> torch.Tensor:
    """``[B, d]`` vectors of the feature tower (differentiable in ``w``); ``weights``: per-bag weight lists or None."""
    rows, d = w.shape
    out = []
    for b, lst in enumerate(lists):
        ws = [1.0] * len(lst) if weights is None else list(weights[b])
        keep = [(int(t), float(x)) for t, x in zip(lst, ws) if 1 <= int(t) < rows]
        wsum = sum(x for _, x in keep)
        if not keep or wsum == 0:
            p = w.sum() * 0 + torch.zeros(d, dtype=w.dtype)
        else:
            wt = torch.tensor([x for _, x in keep], dtype=w.dtype)
            s = (w[torch.tensor([t for t, _ in keep])] * wt[:, None]).sum(0)
            c = {"sum": 1.0, "mean": 1.0 / wsum, "sqrtn": 1.0 / math.sqrt(sum(x * x for _, x in keep))}[combiner]
            p = s * c
        out.append(F.normalize(p, dim=0, eps=1e-12) if normalize else p)
    return torch.stack(out)


def _flat(lists, weights=None):
    flat = torch.tensor([t for x in lists for t in x], dtype=torch.int64)
    off = torch.tensor([0, *torch.tensor([len(x) for x in lists]).cumsum(0)[:-1].tolist()], dtype=torch.int64)
    psw = None if weights is None else torch.tensor([v for x in weights for v in x], dtype=torch.float32)
    return flat, off, psw


def test_spec_sum_with_weights_equals_embedding_bag():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(50, 16, generator=g)
    lists = [torch.randint(0, 50, (n,), generator=g).tolist() for n in (1, 4, 9, 30, 0, 3)]
    lists[1][0] = 0                                               # padding token inside a bag
    weights = [torch.rand(len(x), generator=g).mul(3).tolist() for x in lists]
    flat, off, psw = _flat(lists, weights)
    want = F.embedding_bag(flat, w, off, mode="sum", per_sample_weights=psw, padding_idx=0)
    assert torch.allclose(spec_bag(w, lists, weights, "sum", False), want, atol=1e-5)
    assert torch.allclose(spec_bag(w, lists, weights, "sum", True), F.normalize(want, dim=1, eps=1e-12), atol=1e-5)


def test_spec_unweighted_mean_equals_embedding_bag():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(40, 8, generator=g)
    lists = [torch.randint(0, 40, (n,), generator=g).tolist() for n in (2, 7, 1, 25)] + [[0, 0], []]
    flat, off, _ = _flat(lists)
    want = F.embedding_bag(flat, w, off, mode="mean", padding_idx=0)
    assert torch.allclose(spec_bag(w, lists, None, "mean", False), want, atol=1e-6)


def test_spec_hand_worked_sqrtn_padding_and_empty_bags():
    w = torch.tensor([[9.0, 9.0], [3.0, 4.0], [0.0, 2.0], [1.0, 0.0]])
    # tokens 0 and 4 (>= R = 4) are padding: dropped from the sums AND the weight sums
    lists = [[1, 2, 0, 4], [3, 3], [], [0, 7], [2]]
    weights = [[3.0, 4.0, 100.0, 100.0], [1.0, 1.0], [], [5.0, 5.0], [0.0]]
    p = spec_bag(w, lists, weights, "sqrtn", False)
    # bag 0: (3 * [3, 4] + 4 * [0, 2]) / sqrt(9 + 16) = [9, 20] / 5
    assert torch.allclose(p[0], torch.tensor([1.8, 4.0]))
    assert torch.allclose(p[1], torch.tensor([2.0 / math.sqrt(2.0), 0.0]))
    assert torch.equal(p[2], torch.zeros(2)) and torch.equal(p[3], torch.zeros(2)) and torch.equal(p[4], torch.zeros(2))
    # an fp64 restatement of sqrtn on random bags
    g = torch.Generator().manual_seed(2)
    w = torch.randn(30, 4, generator=g, dtype=torch.float64)
    lists = [torch.randint(1, 30, (n,), generator=g).tolist() for n in (1, 5, 12)]
    weights = [torch.rand(len(x), generator=g, dtype=torch.float64).tolist() for x in lists]
    for b, (lst, ws) in enumerate(zip(lists, weights)):
        s = sum(wt * w[t] for t, wt in zip(lst, ws))
        want = s / math.sqrt(sum(x * x for x in ws))
        assert torch.allclose(spec_bag(w, lists, weights, "sqrtn", False)[b], want)
    # the gradient: w_e * c_b * g on each token's row, nothing for padding, empty or zero-weight bags
    wt = w.clone().requires_grad_(True)
    spec_bag(wt, [[1, 1, 2, 0], [], [3]], [[1.0, 2.0, 4.0, 9.0], [], [0.0]], "mean", False).sum().backward()
    want = torch.zeros_like(w)
    want[1] = 3.0 / 7.0
    want[2] = 4.0 / 7.0
    assert torch.allclose(wt.grad, want)


def _bucket(field, value, n, seed=0):
    h = hashlib.blake2b(f"{field}={value}".encode(), digest_size=8, key=seed.to_bytes(8, "little")).digest()
    return 1 + int.from_bytes(h, "little") % (n - 1)


ITEM = '{"title":"Toy Story (1995)","genres":["Animation","Children\'s","Comedy"]}'
USER = '{"gender":"F","age":1,"occupation":10,"zipcode":"48067"}'


def test_hasher_known_answers_and_reference_json_shapes(mf):
    h = mf.data.FeatureHasher(65535, seed=7)
    assert h.features(ITEM) == ["title=toy", "title=story", "title=1995", "genres=Animation", "genres=Children's",
                                "genres=Comedy"]
    assert h.tokens(ITEM) == [_bucket(*f.split("=", 1), 65535, 7) for f in h.features(ITEM)]
    assert h.features(USER) == ["gender=F", "age=1", "occupation=10", "zipcode=48067"]
    assert h.tokens(json.loads(USER)) == h.tokens(USER)                       # dicts and JSON text alike
    assert h.bucket("genres", "Drama") == _bucket("genres", "Drama", 65535, 7) != _bucket("genres", "Drama", 65535, 8)
    assert h.features({"title": "L'Ãtudiante (1988)"}) == ["title=l", "title=tudiante", "title=1988"]
    assert all(1 <= t < 100 for t in mf.data.FeatureHasher(100).tokens(ITEM))            # bucket 0 is never produced
    hid = mf.data.FeatureHasher(1000, id_field="movie_id")
    bags = hid.bags([ITEM, None], ids=[1, 2])
    assert bags.lists() == [hid.tokens(ITEM) + [_bucket("movie_id", 1, 1000)], [_bucket("movie_id", 2, 1000)]]
    bags = h.bags([None, ITEM, "", USER])
    assert bags.off.tolist() == [0, 0, 6, 6, 10] and bags.max_len == 6 and bags.weights is None


def test_hasher_does_not_depend_on_pythonhashseed(mf):
    code = ("import importlib, json, sys; sys.path.insert(0, sys.argv[1]); "
            "mf = importlib.import_module('matrix-factorization-torch_amd'); "
            f"print(json.dumps(mf.data.FeatureHasher(65535, seed=3).bags([{ITEM!r}, {USER!r}]).lists()))")
    outs = []
    for seed in ("1", "12345"):
        env = {**os.environ, "PYTHONHASHSEED": seed}
        r = subprocess.run([sys.executable, "-c", code, str(ROOT)], env=env, capture_output=True, text=True, check=True)
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1] == mf.data.FeatureHasher(65535, seed=3).bags([ITEM, USER]).lists()


def test_feature_bags_validation(mf):
    B = mf.data.FeatureBags
    with pytest.raises(ValueError, match="finite and >= 0"):
        B([0, 2], [1, 2], [1.0, -0.5])
    with pytest.raises(ValueError, match="finite and >= 0"):
        B([0, 2], [1, 2], [1.0, float("nan")])
    with pytest.raises(ValueError, match="one weight per token"):
        B([0, 2], [1, 2], [1.0])
    with pytest.raises(ValueError, match="offsets"):
        B([0, 3], [1, 2])
    bags = B.from_lists([[3, 4], [], [5]], [[0.5, 1.0], [], [2.0]])
    assert bags.off.tolist() == [0, 2, 2, 3] and bags.max_len == 2 and len(bags) == 3  # noqa: PLR2004
    assert bags.weights.tolist() == [0.5, 1.0, 2.0]


def test_read_movielens_features_rows_match_interactions(mf, tmp_path):
    d1 = tmp_path / "ml-1m"
    d1.mkdir()
    (d1 / "movies.dat").write_bytes("1::Toy Story (1995)::Animation|Children's|Comedy\n5::Heat (1995)::Action|Crime\n"
                                    "3::Cité (1995)::Drama\n".encode("iso-8859-1"))
    (d1 / "users.dat").write_text("2::M::25::7::55117\n1::F::1::10::48067\n")
    (d1 / "ratings.dat").write_text("1::5::4::978300760\n2::1::5::978300761\n1::3::3::978300762\n2::5::2::978300763\n")
    items, users = mf.data.read_movielens_features(d1 / "ratings.dat")
    table, meta = mf.data.movielens_interactions(d1 / "ratings.dat")
    assert len(items) == meta["num_items"] and len(users) == meta["num_users"]
    assert items[0] is None and users[0] is None
    assert items[1] == '{"title":"Toy Story (1995)","genres":["Animation","Children\'s","Comedy"]}'
    assert items[3] == '{"title":"Cité (1995)","genres":["Drama"]}'
    assert users[2] == '{"gender":"F","age":1,"occupation":10,"zipcode":"48067"}'
    # movie 5 / user 1 get rows 2 / 2 in movielens_interactions: the texts at those rows are theirs
    r = mf.data.read_ratings(d1 / "ratings.dat")
    rows = {(int(u), int(m)): None for u, m in zip(r["user_id"], r["movie_id"])}
    assert rows
    assert json.loads(items[2])["title"] == "Heat (1995)" and json.loads(users[1])["zipcode"] == "55117"
    assert int(table.sorted_item.max()) < len(items) and int(table.sorted_user.max()) < len(users)

    d2 = tmp_path / "ml-25m"
    d2.mkdir()
    (d2 / "movies.csv").write_text('movieId,title,genres\n1,Toy Story (1995),Adventure|Animation\n'
                                   '2,"American President, The (1995)",(no genres listed)\n')
    (d2 / "ratings.csv").write_text("userId,movieId,rating,timestamp\n1,2,3.5,1\n1,1,4.0,2\n")
    items, users = mf.data.read_movielens_features(d2 / "ratings.csv")
    assert users is None and len(items) == mf.data.movielens_interactions(d2 / "ratings.csv")[1]["num_items"]
    assert json.loads(items[2]) == {"title": "American President, The (1995)", "genres": ["(no genres listed)"]}


def test_synthetic_item_features(mf):
    texts, genre = mf.data.synthetic_item_features(500, num_genres=10, vocab=100, seed=1)
    assert texts[0] is None and len(texts) == 500 and genre.shape == (500,)  # noqa: PLR2004
    counts = torch.bincount(genre[1:], minlength=10)
    assert counts[0] > 2 * counts[9]                                          # skewed
    for t in texts[1:50]:
        x = json.loads(t)
        words = x["title"].split()
        assert 2 <= len(words) <= 13 and words[-1].startswith("(")  # noqa: PLR2004
        assert x["genres"][0] == f"g{int(genre[texts.index(t)])}"


def test_config_validation_and_refusals(mf):
    M = mf.models.ModelConfig
    with pytest.raises(ValueError, match="needs item_tower='table'"):
        M(user_tower="history", item_tower="features")
    with pytest.raises(ValueError, match="num_hashes"):
        M(item_tower="features", num_hashes=2)
    with pytest.raises(ValueError, match="num_hashes"):
        M(user_tower="features", num_hashes=1)
    with pytest.raises(ValueError, match="2\\^20"):
        M(item_tower="features", feature_buckets=(1 << 20) + 1)
    with pytest.raises(ValueError):
        M(feature_combiner="max")
    with pytest.raises(ValueError):
        M(item_tower="history")
    cfg = mf.lightning.MatrixFactorizationLitConfig(user_tower="features", item_tower="features", feature_combiner="sqrtn",
                                                    feature_seed=3)
    assert mf.lightning.MatrixFactorizationLitConfig.model_validate(json.loads(json.dumps(cfg.model_dump()))) == cfg
    tower = mf.models.FeatureBagTower(100, 32)
    with pytest.raises(ValueError, match="set_bags first"):
        tower(torch.tensor([1]))
    with pytest.raises(ValueError, match="set_bags first"):
        _ = tower.num_embeddings
    with pytest.raises(ValueError, match="combiner"):
        mf.models.FeatureBagTower(100, 32, combiner="max")
    with pytest.raises(ValueError, match="2\\^20"):
        mf.models.FeatureBagTower((1 << 20) + 1, 32)


def test_defaults_leave_init_towers_unchanged(mf):
    cfg = mf.models.ModelConfig(num_users=30, num_items=40, hidden_size=32)
    assert (cfg.item_tower, cfg.user_tower, cfg.feature_buckets, cfg.feature_combiner) == ("table", "table", 65535, "mean")
    torch.manual_seed(0)
    towers = mf.models.init_towers(cfg)
    torch.manual_seed(0)
    want = torch.randn(30, 32) * (1.0 / math.sqrt(32))
    assert type(towers["user"]) is mf.models.EmbeddingTower and type(towers["item"]) is mf.models.EmbeddingTower
    assert torch.equal(towers["user"].weight.detach(), want)
    assert [k for k, _ in towers.named_parameters()] == ["user.weight", "item.weight"]


def test_feature_towers_share_one_table(mf):
    cfg = mf.models.ModelConfig(num_users=30, hidden_size=32, user_tower="features", item_tower="features", feature_buckets=500)
    towers = mf.models.init_towers(cfg)
    user, item = towers["user"], towers["item"]
    assert isinstance(user, mf.models.FeatureBagTower) and isinstance(item, mf.models.FeatureBagTower)
    assert user.weight is item.weight and item.weight.shape == (500, 32)
    assert [p is item.weight for p in towers.parameters()] == [True]
    assert list(towers.state_dict()) == ["item.weight"]
    mixed = mf.models.init_towers(mf.models.ModelConfig(num_users=30, hidden_size=32, item_tower="features", feature_buckets=500))
    assert type(mixed["user"]) is mf.models.EmbeddingTower and mixed["user"].weight.shape == (30, 32)
    assert isinstance(mixed["item"], mf.models.FeatureBagTower)


def test_bag_and_coalesce_kernels_do_not_spill(mf):
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = kr.kernel_resources()
    mine = {k: v for k, v in res.items() if "bag_" in k or "coalesce_" in k}
    assert len(mine) >= 29, sorted(mine)  # noqa: PLR2004
    for k, v in mine.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, k
        assert v["private_segment_fixed_size"] == 0, k
