"""GPU: the transformer tower's serving encode (HistoryTransformerTower.encode; mf_xfmr_encode: one launch, one workgroup per
user, no stash) against the training forward it must equal BIT FOR BIT at fp32, and -- independently of that forward -- against
the plain-torch spec of tests/test_xfmr_tower_cpu.py under the tower's standing rule: the reference is the spec in fp64, the
fp32 CPU spec's own error against it is measured on the same inputs, and the kernel may err up to 8 x that plus 1e-7, max-abs
over the max-abs of the fp64 value.  Every figure is printed before it is asserted (``pytest -s``)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from tests.test_xfmr_tower_cpu import HARD_CASES, hard_case, random_state, spec_tower

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ROWS = 300
SIZES = [0, 1, 5, 31, 32, 33, 63, 64, 65, 130]
ACTS = ("gelu", "relu", "silu", "gelu_new")
MODES = ("mean", "max", "cls")


def _check(name: str, got: torch.Tensor, spec32: torch.Tensor, ref64: torch.Tensor) -> None:
    assert bool(torch.isfinite(got).all()), name
    ref = ref64.double().cpu()
    scale = max(float(ref.abs().max()), 1e-30)
    e_k = float((got.double().cpu() - ref).abs().max()) / scale
    e_s = float((spec32.double().cpu() - ref).abs().max()) / scale
    print(f"  {name}: kernel {e_k:.3e}  fp32 spec {e_s:.3e}  ratio {e_k / e_s if e_s > 0 else float('inf' if e_k else 0):.2f}")
    assert e_k <= FACTOR * e_s + 1e-7, (name, e_k, e_s)


def _segments(lists):
    off = torch.tensor(np.cumsum([0] + [len(x) for x in lists]), dtype=torch.int64, device=DEV)
    items = torch.tensor([i for x in lists for i in x] or [0], dtype=torch.int64, device=DEV)
    return off[:-1], off[1:], items


def _padded(lists):
    width = max(1, max(len(x) for x in lists))
    pad = torch.zeros(len(lists), width, dtype=torch.int64)
    for b, x in enumerate(lists):
        if x:
            pad[b, width - len(x):] = torch.tensor(x)
    return pad.to(DEV)


def _lists(rng, n_rows, sizes):
    """Lists with a padding zero, an out-of-range id (negative or >= n_rows) and a repeat at entries 1, 2, 3 of every list of
    four or more -- where ``_lists`` of tests/test_gpu_xfmr_tower.py places them."""
    out = []
    for k, n in enumerate(sizes):
        lst = rng.integers(1, n_rows, n).tolist()
        if n >= 4:  # noqa: PLR2004
            lst[1] = 0
            lst[2] = -3 if k % 2 else n_rows + 5
            lst[3] = lst[0]
        out.append(lst)
    return out


def _world(seed, rows, h, layers, inter, max_pos=64):
    g = torch.Generator().manual_seed(seed)
    sd = random_state(g, h, layers, inter, max_pos, dtype=torch.float64)
    w = torch.randn(rows, h, generator=g, dtype=torch.float64) / h ** 0.5
    return w, sd


def _towers(mf, w, sd, *, heads, act, mode, L, n_i=True, n_u=True, **kw):
    rows, h = w.shape
    layers = sum(k.endswith("attention.self.query.weight") for k in sd)
    item = mf.models.EmbeddingTower(rows, h, normalize=n_i, device=DEV)
    with torch.no_grad():
        item.weight.copy_(w.float())
    user = mf.models.HistoryTransformerTower(item, num_hidden_layers=layers, num_attention_heads=heads,
                                             intermediate_size=sd["encoder.layer.0.intermediate.dense.weight"].shape[0], hidden_act=act,
                                             max_position_embeddings=sd["embeddings.position_embeddings.weight"].shape[0],
                                             pooling_mode=mode, max_history=L, normalize=n_u, **kw)
    user.load_state_dict({k: v.float() for k, v in sd.items()})
    return item, user


def _export(mf, user, history):
    """``mf_xfmr_encode`` called directly, on the caller's buffers (the output poisoned first)."""
    lib = mf._lib.lib()
    start, end, items, _ = user.segments(history)
    params = [p.detach() for p in user.encoder_parameters()]
    table = user.weight.detach()
    rows, d = table.shape
    out = torch.full((start.numel(), d), float("nan"), device=DEV)
    arr = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
    rc = lib.mf_xfmr_encode(table.data_ptr(), rows, d, start.data_ptr(), end.data_ptr(), items.data_ptr(), items.numel(), start.numel(),
                            user.max_history, user.num_hidden_layers, user.num_attention_heads, user.intermediate_size,
                            ACTS.index(user.hidden_act), MODES.index(user.pooling_mode), int(user.item_tower.normalize),
                            int(user.normalize), arr, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mf_last_error().decode()
    return out


# (h, heads, L, intermediate, layers, act, mode): every h, head width 8 / 16 / 32 / 64 (16 heads at h = 128), L in {1, 7, 16, 33,
# 64}, I in {32, 96, h, 4 h} (I < h, a non-multiple of 64, 512), 1 / 2 / 4 layers, every activation and pooling mode
CASES = [
    (32, 4, 1, 32, 1, "gelu", "mean"), (32, 2, 7, 96, 2, "relu", "max"), (32, 1, 16, 128, 4, "silu", "cls"),
    (32, 4, 33, 32, 1, "gelu_new", "mean"), (64, 8, 64, 64, 2, "gelu", "max"), (64, 4, 33, 96, 1, "relu", "cls"),
    (64, 2, 16, 256, 4, "silu", "mean"), (64, 1, 64, 32, 1, "gelu_new", "max"), (128, 16, 64, 512, 1, "gelu", "mean"),
    (128, 8, 33, 96, 2, "relu", "cls"), (128, 4, 7, 128, 4, "silu", "max"), (128, 2, 64, 512, 2, "gelu_new", "mean"),
    (128, 4, 1, 32, 1, "gelu", "cls"), (64, 4, 7, 64, 1, "silu", "max"), (128, 4, 16, 512, 1, "relu", "max"),
]
NORM_FORMS = ((True, True, False), (False, True, True), (True, False, True), (False, False, False))    # n_i, n_u, padded
_ids = lambda c: "-".join(str(x) for x in c)  # noqa: E731


def test_cases_cover_every_axis():
    assert {c[0] for c in CASES} == {32, 64, 128}
    assert {c[0] // c[1] for c in CASES} == {8, 16, 32, 64} and (128, 16) in {c[:2] for c in CASES}
    assert {c[2] for c in CASES} == {1, 7, 16, 33, 64}
    for h in (32, 64, 128):
        assert {32, 96, h, 4 * h} <= {c[3] for c in CASES if c[0] == h}
    assert {c[4] for c in CASES} == {1, 2, 4}
    assert {c[5] for c in CASES} == set(ACTS) and {c[6] for c in CASES} == set(MODES)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fused_is_bit_identical_to_the_forward(mf, case):
    h, heads, L, inter, layers, act, mode = case
    rng = np.random.default_rng(h + L + inter)
    w, sd = _world(h + heads + layers, ROWS, h, layers, inter)
    lists = _lists(rng, ROWS, SIZES)
    for k, (n_i, n_u, padded) in enumerate(NORM_FORMS):
        _, user = _towers(mf, w, sd, heads=heads, act=act, mode=mode, L=L, n_i=n_i, n_u=n_u)
        hist = _padded(lists) if padded else _segments(lists)
        fused, fwd = user.encode(hist, path="fused"), user.encode(hist, path="forward")
        with torch.no_grad():
            plain = user.eval()(hist)
        assert torch.equal(fwd, plain)
        assert fused.shape == (len(lists), h) and torch.equal(fused, fwd), (case, n_i, n_u, padded, float((fused - fwd).abs().max()))
        assert torch.equal(fused[0].cpu(), torch.zeros(h))                   # the empty list: exactly zero
        assert bool((fused[1:].abs().sum(1) > 0).all())
        if k % 2 == 0:
            assert torch.equal(_export(mf, user, hist), fwd)
        other = _segments(lists) if padded else _padded(lists)              # the other input form: the same bits
        if k == 1:
            assert torch.equal(user.encode(other, path="fused"), fwd)


SPEC_CASES = [CASES[1], CASES[4], CASES[7], CASES[8], CASES[11], CASES[2]]


@pytest.mark.parametrize("case", SPEC_CASES, ids=_ids)
def test_fused_matches_the_spec(mf, case):
    h, heads, L, inter, layers, act, mode = case
    rng = np.random.default_rng(h + L)
    w, sd = _world(h + heads, ROWS, h, layers, inter)
    lists = _lists(rng, ROWS, SIZES)
    sd32 = {k: v.float() for k, v in sd.items()}
    for n_i, n_u, padded in NORM_FORMS[:2] if layers > 1 else NORM_FORMS:
        _, user = _towers(mf, w, sd, heads=heads, act=act, mode=mode, L=L, n_i=n_i, n_u=n_u)
        got = user.encode(_padded(lists) if padded else _segments(lists), path="fused")
        kw = {"heads": heads, "act": act, "mode": mode, "n_i": n_i, "n_u": n_u, "max_history": L}
        _check(f"u {case} n_i={n_i} n_u={n_u} padded={padded}", got, spec_tower(w.float(), lists, sd32, **kw), spec_tower(w, lists, sd, **kw))


# one of every hard world at h = 128 and head widths 8 / 64, two layers, I < h and I = 2 h
HARD = [c for c in HARD_CASES if c in (("sharp", 128, 16, 64, "max", 1, "gelu", 64), ("sharp", 64, 1, 64, "max", 1, "gelu", 64),
                                       ("saturated", 128, 4, 64, "max", 1, "silu", 256), ("saturated", 64, 8, 64, "mean", 2, "silu", 160),
                                       ("offset", 128, 8, 64, "max", 1, "silu", 128), ("flat", 128, 4, 64, "mean", 2, "relu", 128))]


def test_hard_selection_holds_the_four_worlds():
    assert len(HARD) == 6 and {c[0] for c in HARD} == {"sharp", "saturated", "offset", "flat"}  # noqa: PLR2004


@pytest.mark.parametrize("case", HARD, ids=_ids)
def test_hard_worlds_match_the_spec(mf, case):
    w, sd, lists, _, kw = hard_case(*case)
    _, user = _towers(mf, w, sd, heads=kw["heads"], act=kw["act"], mode=kw["mode"], L=kw["max_history"], n_i=kw["n_i"], n_u=kw["n_u"])
    sd32 = {k: v.float() for k, v in sd.items()}
    s32, ref = spec_tower(w.float(), lists, sd32, **kw), spec_tower(w, lists, sd, **kw)
    for padded in (False, True):
        hist = _padded(lists) if padded else _segments(lists)
        got = user.encode(hist, path="fused")
        _check(f"u {case} padded={padded}", got, s32, ref)
        assert torch.equal(got, user.encode(hist, path="forward"))


def _sparse_list(rng, n_rows, length, n_valid=None):
    """``length`` ids with one valid id at a random place of every three entries (``n_valid``: with exactly that many valid ids, at
    random places); every other id is 0, negative or >= ``n_rows``."""
    if n_valid is None:
        keep = {3 * g + int(rng.integers(0, 3)) for g in range(length // 3)}
    else:
        keep = set(rng.choice(length, n_valid, replace=False).tolist())
    bad = lambda: (0, -int(rng.integers(1, 1000)), n_rows + int(rng.integers(0, 1000)))[int(rng.integers(0, 3))]  # noqa: E731
    return [int(rng.integers(1, n_rows)) if i in keep else bad() for i in range(length)]


def test_long_sparse_lists_pack_the_same_tokens(mf):
    """The pack walk (``list_pack_walk``: shared by ``xfmr_pack_kernel`` and the encode kernel's wave 0) over lists whose kept
    entries lie far apart: the last 64 valid of 66 among 200 entries, exactly 64 and 63 valid among 150, and an empty list."""
    h, heads, L, inter = 32, 4, 64, 32
    rng = np.random.default_rng(64)
    lists = [_sparse_list(rng, ROWS, 200), _sparse_list(rng, ROWS, 200), _sparse_list(rng, ROWS, 150, 64), _sparse_list(rng, ROWS, 150, 63), []]
    kept = [[i for i, x in enumerate(lst) if 1 <= x < ROWS][-L:] for lst in lists]       # the entries the spec keeps, by place
    assert [len(k) for k in kept] == [64, 64, 64, 63, 0]
    for lst, k in zip(lists[:2], kept[:2]):
        assert len(lst) == 200 and sum(1 <= x < ROWS for x in lst) == 66  # noqa: PLR2004
        assert any(x == 0 for x in lst) and any(x < 0 for x in lst) and any(x >= ROWS for x in lst)
        assert len({(len(lst) - 1 - i) // 64 for i in k}) >= 3  # noqa: PLR2004  (blocks of the cut's walk, from the end)
        assert len({(i - k[0]) // 64 for i in k}) >= 3  # noqa: PLR2004          (blocks of the pack's walk, from the cut)
    w, sd = _world(21, ROWS, h, 1, inter)
    _, user = _towers(mf, w, sd, heads=heads, act="gelu", mode="mean", L=L)
    kw = {"heads": heads, "act": "gelu", "mode": "mean", "n_i": True, "n_u": True, "max_history": L}
    s32, ref = spec_tower(w.float(), lists, {k: v.float() for k, v in sd.items()}, **kw), spec_tower(w, lists, sd, **kw)
    hist = _segments(lists)
    fused, fwd = user.encode(hist, path="fused"), user.encode(hist, path="forward")
    assert torch.equal(fused, fwd), float((fused - fwd).abs().max())
    assert torch.equal(fused[4].cpu(), torch.zeros(h)) and bool((fused[:4].abs().sum(1) > 0).all())
    _check("u fused, long sparse lists", fused, s32, ref)
    _check("u forward, long sparse lists", fwd, s32, ref)


def test_batch_shapes(mf):
    w, sd = _world(5, ROWS, 32, 1, 32)
    _, user = _towers(mf, w, sd, heads=4, act="gelu", mode="mean", L=16)
    one = _segments([[7, 9, 0, 11]])
    u1 = user.encode(one, path="fused")
    assert u1.shape == (1, 32) and torch.equal(u1, user.encode(one, path="forward")) and float(u1.abs().sum()) > 0
    pad = torch.tensor([[0, -1, ROWS, ROWS + 7], [0, 0, 0, 0], [-5, 0, ROWS, 0]], dtype=torch.int64, device=DEV)
    for hist in (pad, _segments(pad.tolist()), _segments([[], [], []])):
        z = user.encode(hist, path="fused")
        assert z.shape == (3, 32) and torch.equal(z.cpu(), torch.zeros(3, 32))
    rng = np.random.default_rng(3)
    many = [rng.integers(1, ROWS, int(n)).tolist() for n in rng.integers(0, 4, 3000)]    # more workgroups than CUs
    hist = _segments(many)
    big = user.encode(hist, path="fused")
    assert big.shape == (3000, 32) and torch.equal(big, user.encode(hist, path="forward"))
    empty = torch.tensor([len(x) == 0 for x in many])
    assert bool(empty.any()) and torch.equal(big.cpu()[empty], torch.zeros(int(empty.sum()), 32))
    assert bool((big.cpu()[~empty].abs().sum(1) > 0).all())


def test_mode_and_state(mf):
    w, sd = _world(11, ROWS, 64, 2, 96)
    item, user = _towers(mf, w, sd, heads=4, act="gelu", mode="mean", L=16, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                         dropout_seed=5)
    user.train()
    hist = _segments(_lists(np.random.default_rng(0), ROWS, [1, 9, 16, 40, 0]))
    with torch.no_grad():
        dropped = user(hist)                                                  # a training forward: drops, advances the counter
    assert user.dropout_call == 1
    before = {k: v.detach().clone() for k, v in user.state_dict().items()}
    table = item.weight.detach().clone()
    got = {path: user.encode(hist, path=path) for path in ("fused", "forward", "auto")}   # no torch.no_grad() around it
    assert user.training and user.dropout_call == 1
    for u in got.values():
        assert u.grad_fn is None and not u.requires_grad
    assert getattr(item.weight, "_mf_pending", None) in (None, [])
    assert torch.equal(item.weight.detach(), table)
    for k, v in user.state_dict().items():
        assert torch.equal(v, before[k]), k
    user.eval()
    with torch.no_grad():
        want = user(hist)
    user.train()
    assert not torch.equal(want, dropped)
    for path, u in got.items():
        assert torch.equal(u, want), path
    with pytest.raises(ValueError, match="path"):
        user.encode(hist, path="quick")


def test_bf16_mixed_tower_keeps_its_precision(mf):
    w, sd = _world(12, ROWS, 64, 1, 128)
    _, mixed = _towers(mf, w, sd, heads=4, act="gelu", mode="mean", L=16, precision="bf16-mixed")
    _, plain = _towers(mf, w, sd, heads=4, act="gelu", mode="mean", L=16)
    hist = _segments(_lists(np.random.default_rng(1), ROWS, [3, 16, 20]))
    mixed.eval()
    with torch.no_grad():
        want = mixed(hist)
    assert torch.equal(mixed.encode(hist), want) and torch.equal(mixed.encode(hist, path="forward"), want)
    assert not torch.equal(want, plain.encode(hist))                          # (the mixed function is another function)
    with pytest.raises(ValueError, match="fp32"):
        mixed.encode(hist, path="fused")


def test_auto_follows_the_threshold(mf, monkeypatch):
    w, sd = _world(13, ROWS, 32, 1, 32)
    _, user = _towers(mf, w, sd, heads=4, act="gelu", mode="mean", L=8)
    lib = mf._lib.lib()
    calls = []
    real = lib.mf_xfmr_encode
    monkeypatch.setattr(lib, "mf_xfmr_encode", lambda *a: calls.append(a[7]) or real(*a))
    hist = _padded([[1, 2, 3]] * 5)
    for limit, used in ((None, True), (5, True), (4, False)):
        monkeypatch.setattr(mf.models, "XFMR_ENCODE_FUSED_MAX_USERS", limit)
        calls.clear()
        u = user.encode(hist)
        assert bool(calls) == used and torch.equal(u, user.encode(hist, path="forward"))


def test_no_per_token_memory(mf):
    b, L, h, inter = 512, 64, 128, 512
    w, sd = _world(14, ROWS, h, 1, inter)
    _, user = _towers(mf, w, sd, heads=4, act="gelu", mode="mean", L=L)
    hist = torch.randint(1, ROWS, (b, L), device=DEV)
    user.encode(hist, path="fused")                                           # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    u = user.encode(hist, path="fused")
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    stash = mf._lib.lib().mf_xfmr_ws_bytes(b, b * L, h, 1, inter)
    print(f"  fused encode: {rise} bytes above the baseline; the forward's stash is {stash} bytes")
    assert u.numel() * 4 <= rise < stash // 4
    assert not hasattr(mf._lib.lib(), "mf_xfmr_encode_ws_bytes")              # no scratch beyond LDS: nothing to size


def test_module_serves_through_the_export(mf, monkeypatch):
    cfg = {"num_users": 40, "num_items": 60, "hidden_size": 32, "learning_rate": 0.02, "user_tower": "transformer", "max_history": 8,
           "num_negatives": 2, "train_loss": "InfomationNoiseContrastiveEstimationLoss", "top_k": 10, "hidden_dropout_prob": 0.1}
    m = mf.lightning.MatrixFactorizationLitModule(cfg)
    m.configure_model(device=DEV)
    m.train()
    m.item_processor.get_index(m)
    tower, proc = m.towers["user"], m.item_processor
    lib = mf._lib.lib()
    count = [0]
    real = lib.mf_xfmr_encode

    def counting(*a):
        count[0] += 1
        return real(*a)

    monkeypatch.setattr(lib, "mf_xfmr_encode", counting)
    hist = [3, 7, 7, 11, 20]
    want = proc.search(tower.encode(torch.tensor([hist], device=DEV), path="forward").cpu().numpy(), exclude_item_ids=hist, top_k=10)
    assert count[0] == 0
    rec = m.recommend_with_history(hist, top_k=10)
    assert count[0] == 1
    assert rec["movie_rn"].tolist() == want["movie_rn"].tolist() and rec["score"].tolist() == want["score"].tolist()
    m.history = {5: hist}
    rec = m.recommend(5, top_k=10)
    assert count[0] == 2  # noqa: PLR2004
    assert rec["movie_rn"].tolist() == want["movie_rn"].tolist() and rec["score"].tolist() == want["score"].tolist()
    off = torch.tensor([0, 3, 3, 8], device=DEV)
    items = torch.tensor([4, 9, 2, 7, 7, 1, 30, 12], device=DEV)
    ev = {"user": {"idx": torch.tensor([1, 2, 3], device=DEV)}, "history": (off, items)}
    scores, rows = m.predict_step(ev)
    assert count[0] == 3  # noqa: PLR2004
    q = tower.encode((off[:-1], off[1:], items), path="forward")
    want_scores, want_rows = proc.index.search(q, 10, exclude_csr=ev["history"])
    assert torch.equal(scores, want_scores) and torch.equal(rows, want_rows)
    assert tower.training and tower.dropout_call == 0
