"""CPU: the training dropout of the transformer user tower.  The mask generator of ``include/mf_numerics.h`` restated in numpy
(held to the header's known answers and to the library's host export ``mf_dropout_words``), its statistics, the dropout spec
``spec_tower_dropout`` (``tests/test_xfmr_tower_cpu.py``'s encoder with BertModel's four dropout sites, masks from the numpy
generator -- the GPU tests hold the kernels to it), and the configuration surface."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_xfmr_tower_cpu import ACTS, random_state, rel_err, spec_encoder, spec_pool, spec_step, spec_tower

MASK64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
STREAM_EMBEDDINGS = 16


# ------------------------------------------------------------------------------------- the generator ----
def splitmix64(z: np.ndarray) -> np.ndarray:
    """SplitMix64's output function on uint64 arrays (array arithmetic wraps)."""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u64(x: int) -> np.ndarray:
    return np.array([x & MASK64], dtype=np.uint64)


def dropout_key(seed: int, call: int, stream: int) -> int:
    inner = splitmix64(_u64(seed + GAMMA * (call + 1)))
    return int(splitmix64(_u64(int(inner[0]) + GAMMA * (stream + 1)))[0])


def dropout_words(key: int, idx) -> np.ndarray:
    idx = np.asarray(idx, dtype=np.uint64)
    return splitmix64(np.uint64(key) + idx * np.uint64(GAMMA))


def fields(words: np.ndarray) -> np.ndarray:
    """``[..., 4]``: field f = (word >> 16 f) & 0xFFFF."""
    return (words[..., None] >> (np.arange(4, dtype=np.uint64) * np.uint64(16))) & np.uint64(0xFFFF)


def threshold(p: float) -> int:
    return min(int(math.floor(p * 65536.0 + 0.5)), 65535)


def hidden_keep(seed: int, call: int, stream: int, b: int, n: int, h: int, thr: int) -> torch.Tensor:
    """``[n, h]`` bool: element (user b, position t, column c) is field c & 3 of word (b 64 + t) 32 + c / 4."""
    t, c = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(h, dtype=np.uint64), indexing="ij")
    words = dropout_words(dropout_key(seed, call, stream), (np.uint64(b * 64) + t) * np.uint64(32) + (c >> np.uint64(2)))
    f = (words >> ((c & np.uint64(3)) * np.uint64(16))) & np.uint64(0xFFFF)
    return torch.from_numpy(f >= np.uint64(thr))


def attn_keep(seed: int, call: int, stream: int, b: int, n: int, heads: int, thr: int) -> torch.Tensor:
    """``[heads, n, n]`` bool (head, query i, key j): field j & 3 of word ((b 64 + i) 16 + head) 16 + j / 4."""
    hd, i, j = np.meshgrid(np.arange(heads, dtype=np.uint64), np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64), indexing="ij")
    idx = ((np.uint64(b * 64) + i) * np.uint64(16) + hd) * np.uint64(16) + (j >> np.uint64(2))
    words = dropout_words(dropout_key(seed, call, stream), idx)
    f = (words >> ((j & np.uint64(3)) * np.uint64(16))) & np.uint64(0xFFFF)
    return torch.from_numpy(f >= np.uint64(thr))


def scale_of(thr: int, dtype) -> torch.Tensor:
    """1 / (1 - thr / 65536) in ``dtype`` (fp32: the kernels' arithmetic; thr / 65536 and the difference are exact)."""
    one = torch.ones((), dtype=dtype)
    return one / (one - torch.tensor(thr, dtype=dtype) / 65536)


# ------------------------------------------------------------------------------------------ the spec ----
def spec_encoder_dropout(x: torch.Tensor, sd: dict, *, heads: int, act: str, b: int, thr_hidden: int, thr_attn: int, seed: int, call: int,
                         prefix: str = "", trace: dict | None = None) -> torch.Tensor:
    """``spec_encoder`` in train mode for user ``b`` of the call's batch: BertModel's dropout after the embedding LayerNorm,
    on the attention probabilities, and on the attention-output and FFN-output dense results before their residual adds.
    A site whose threshold is 0 is skipped.  ``trace`` receives every layer's context rows ("ctx") and masks."""
    n, h = x.shape
    dh = h // heads
    dt = x.dtype

    def p(name):
        return sd[prefix + name]

    def ln(v, name):
        return F.layer_norm(v, (h,), p(name + ".weight"), p(name + ".bias"), 1e-12)

    def dense(v, name):
        return F.linear(v, p(name + ".weight"), p(name + ".bias"))

    def note(key, v):
        if trace is not None:
            trace.setdefault(key, []).append(v.detach() if v.dtype.is_floating_point else v)
        return v

    def drop_hidden(v, stream):
        if thr_hidden == 0:
            return v
        keep = note("hidden_keep", hidden_keep(seed, call, stream, b, n, h, thr_hidden))
        return v * (keep.to(dt) * scale_of(thr_hidden, dt))

    e = drop_hidden(ln((x + p("embeddings.token_type_embeddings.weight")[0]) + p("embeddings.position_embeddings.weight")[:n],
                       "embeddings.LayerNorm"), STREAM_EMBEDDINGS)
    layer = 0
    while f"{prefix}encoder.layer.{layer}.attention.self.query.weight" in sd:
        base = f"encoder.layer.{layer}."
        q, k, v = (dense(e, f"{base}attention.self.{name}").view(n, heads, dh).transpose(0, 1) for name in ("query", "key", "value"))
        prob = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
        if thr_attn:
            keep = note("attn_keep", attn_keep(seed, call, 4 * layer + 0, b, n, heads, thr_attn))
            prob = prob * (keep.to(dt) * scale_of(thr_attn, dt))
        ctx = note("ctx", (prob @ v).transpose(0, 1).reshape(n, h))
        note("v", v.transpose(0, 1).reshape(n, h))
        y1 = ln(drop_hidden(dense(ctx, f"{base}attention.output.dense"), 4 * layer + 1) + e, f"{base}attention.output.LayerNorm")
        f = ACTS[act](dense(y1, f"{base}intermediate.dense"))
        e = ln(drop_hidden(dense(f, f"{base}output.dense"), 4 * layer + 2) + y1, f"{base}output.LayerNorm")
        layer += 1
    return e


def spec_tower_dropout(w: torch.Tensor, lists, sd: dict, *, heads: int, act: str, mode: str, n_i: bool, n_u: bool, max_history: int,
                       p_hidden: float, p_attn: float, seed: int, call: int, prefix: str = "", trace: dict | None = None) -> torch.Tensor:
    """``spec_tower`` in train mode: user b of ``lists`` is user b of the masks."""
    rows, d = w.shape
    thr_h, thr_a = threshold(p_hidden), threshold(p_attn)
    out = []
    for b, lst in enumerate(lists):
        valid = [int(i) for i in lst if 1 <= int(i) < rows][-max_history:]
        if not valid:
            out.append(w.sum() * 0 + torch.zeros(d, dtype=w.dtype))
            continue
        x = w[torch.tensor(valid)]
        if n_i:
            x = F.normalize(x, dim=1, eps=1e-12)
        y = spec_encoder_dropout(x, sd, heads=heads, act=act, b=b, thr_hidden=thr_h, thr_attn=thr_a, seed=seed, call=call, prefix=prefix,
                                 trace=trace)
        out.append(spec_pool(y, mode, n_u))
    return torch.stack(out)


def spec_step_dropout(w, sd, lists, c, kw, extra, lr, dtype, drop):
    """``spec_step`` through ``spec_tower_dropout``; ``drop``: p_hidden, p_attn, seed, call."""
    wl = w.to(dtype).clone().requires_grad_(True)
    leaf = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    u = spec_tower_dropout(wl, lists, leaf, **kw, **drop)
    loss = (u * c.to(dtype)).sum()
    if extra is not None:
        ids, c2 = extra
        v = wl[ids]
        loss = loss + ((F.normalize(v, dim=1, eps=1e-12) if kw["n_i"] else v) * c2.to(dtype)).sum()
    loss.backward()
    delta = (wl.detach() - lr * wl.grad) - wl.detach()
    return u.detach(), delta, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}


def dropout_lists(rng, rows: int, L: int, users: int = 37) -> list:
    """``users`` lists with lengths 0, 1, L, L + 7 and random ones up to L + 10; padding zeros, out-of-range ids, repeats."""
    sizes = [0, 1, L, L + 7] + rng.integers(0, L + 11, users - 4).tolist()
    out = []
    for k, n in enumerate(sizes):
        lst = rng.integers(1, rows, n).tolist()
        if n >= 4:  # noqa: PLR2004
            lst[1] = lst[0]
            lst.insert(2, 0 if k % 2 else rows + 3)
        out.append(lst)
    return out


# --------------------------------------------------------------------------------------------- tests ----
def test_known_answers():
    assert int(splitmix64(_u64(GAMMA))[0]) == 0xE220A8397B1DCDAF              # SplitMix64's first output (the hash towers' pin)
    key = dropout_key(0, 0, 0)
    assert key == 0xA706DD2F4D197E6F
    assert int(dropout_words(key, [0])[0]) == 0xB49AB477BB8685E2
    assert fields(dropout_words(key, [0]))[0].tolist() == [0x85E2, 0xBB86, 0xB477, 0xB49A]
    assert [threshold(p) for p in (0.0, 0.1, 0.5, 0.9375, 0.5 / 65536, 1 - 2.0 ** -17, 1e-6)] == [0, 6554, 32768, 61440, 1, 65535, 0]


@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("stream", [0, 3, 16])
def test_library_words_equal_the_restatement(mf, seed, stream):
    lib = mf._lib.lib()
    n = 4096
    for call, idx0 in ((0, 0), (5, (37 * 64 + 63) * 32), (2 ** 40 + 1, 2 ** 35)):
        out = np.zeros(n, dtype=np.uint64)
        assert lib.mf_dropout_words(seed, call, stream, idx0, n, out.ctypes.data) == 0
        want = dropout_words(dropout_key(seed, call, stream), np.arange(idx0, idx0 + n, dtype=np.uint64))
        assert np.array_equal(out, want), (call, idx0)
    assert lib.mf_dropout_words(seed, 0, stream, 0, 4, None) == mf._lib.MF_EINVAL
    assert mf.models.dropout_threshold(0.1) == threshold(0.1) and mf.models.dropout_threshold(1 - 2.0 ** -17) == 65535  # noqa: PLR2004


STAT_KEYS = [(0, 0, 0), (1, 0, 0), (0, 1, 3), (12345, 7, 16)]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize(("seed", "call", "stream"), STAT_KEYS)
def test_keep_rate_and_neighbour_correlation(seed, call, stream, p):
    """2^18 words x 4 fields: the kept share is within 5 sigma of 1 - thr / 65536, sigma = sqrt(p (1 - p) / n); the
    correlation of neighbouring fields (in element order), scaled by sqrt(n), is below 5."""
    thr = threshold(p)
    q = thr / 65536.0
    keep = (fields(dropout_words(dropout_key(seed, call, stream), np.arange(1 << 18, dtype=np.uint64))) >= thr).reshape(-1).astype(np.float64)
    n = keep.size
    assert n == 1 << 20
    sigma = math.sqrt(q * (1 - q) / n)
    dev = abs(keep.mean() - (1 - q)) / sigma
    a, b = keep[:-1] - keep.mean(), keep[1:] - keep.mean()
    corr = float((a * b).mean() / keep.var()) * math.sqrt(n)
    print(f"seed={seed} call={call} stream={stream} p={p}: keep rate off by {dev:.2f} sigma, neighbour correlation x sqrt(n) = {corr:.2f}")
    assert dev <= 5.0 and abs(corr) < 5.0  # noqa: PLR2004


def _world(dtype, layers=2):
    g = torch.Generator().manual_seed(4)
    rows, h = 60, 32
    sd = random_state(g, h, layers, 64, 16, dtype=torch.float64)
    w = torch.randn(rows, h, generator=g, dtype=torch.float64) / h ** 0.5
    lists = dropout_lists(np.random.default_rng(4), rows, 8, users=9)
    c = torch.randn(len(lists), h, generator=g, dtype=torch.float64)
    kw = {"heads": 4, "act": "gelu", "mode": "mean", "n_i": True, "n_u": True, "max_history": 8}
    return w.to(dtype), {k: v.to(dtype) for k, v in sd.items()}, lists, c, kw


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_spec_without_dropout_is_the_eval_spec(dtype):
    w, sd, lists, c, kw = _world(dtype)
    off = {"p_hidden": 0.0, "p_attn": 0.0, "seed": 3, "call": 9}
    for mode in ("mean", "max", "cls"):
        assert torch.equal(spec_tower_dropout(w, lists, sd, **{**kw, "mode": mode}, **off), spec_tower(w, lists, sd, **{**kw, "mode": mode}))
    got, want = spec_step_dropout(w, sd, lists, c, kw, None, 0.5, dtype, off), spec_step(w, sd, lists, c, kw, None, 0.5, dtype)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert all(torch.equal(got[2][k], want[2][k]) for k in want[2])
    x = F.normalize(w[torch.tensor([3, 4, 5])], dim=1, eps=1e-12)
    assert torch.equal(spec_encoder_dropout(x, sd, heads=4, act="gelu", b=2, thr_hidden=0, thr_attn=0, seed=0, call=0),
                       spec_encoder(x, sd, heads=4, act="gelu"))


def test_spec_masks_are_the_same_bits_in_both_dtypes():
    drop = {"p_hidden": 0.3, "p_attn": 0.2, "seed": 11, "call": 2}
    traces = []
    for dtype in (torch.float32, torch.float64):
        w, sd, lists, _, kw = _world(dtype)
        tr: dict = {}
        u = spec_tower_dropout(w, lists, sd, **kw, **drop, trace=tr)
        assert bool(torch.isfinite(u).all())
        traces.append((tr, u))
    (t32, u32), (t64, u64) = traces
    for key in ("hidden_keep", "attn_keep"):
        assert len(t32[key]) == len(t64[key]) > 0
        assert all(torch.equal(a, b) for a, b in zip(t32[key], t64[key]))
        kept = torch.cat([m.flatten() for m in t32[key]]).float().mean()
        assert 0.5 < float(kept) < 0.95, key                                   # noqa: PLR2004
    w, sd, lists, _, kw = _world(torch.float64)
    assert rel_err(u32, u64) < 1e-4 and float((u64 - spec_tower(w, lists, sd, **kw)).abs().max()) > 1e-2  # noqa: PLR2004
    # another call, another seed and another user index: other masks
    for other in ({**drop, "call": 3}, {**drop, "seed": 12}):
        assert float((spec_tower_dropout(w, lists, sd, **kw, **other) - u64).abs().max()) > 1e-3  # noqa: PLR2004
    same_list_twice = [lists[2], lists[2]]
    u2 = spec_tower_dropout(w, same_list_twice, sd, **kw, **drop)
    assert float((u2[0] - u2[1]).abs().max()) > 1e-3                         # noqa: PLR2004


def test_spec_hand_worked_single_token():
    """One user, one token, h = 32, one head: the softmax is 1, so the attention mask either keeps the single key
    (ctx = scale v) or drops it (ctx = 0).  One seed for each outcome, picked from the generator."""
    g = torch.Generator().manual_seed(2)
    h, p_attn = 32, 0.5
    thr = threshold(p_attn)
    sd = random_state(g, h, 1, 32, 4, dtype=torch.float64)
    w = torch.randn(6, h, generator=g, dtype=torch.float64)
    first = {seed: int(fields(dropout_words(dropout_key(seed, 0, 0), [0]))[0, 0]) for seed in range(64)}     # (b, i, head, j) = 0: word 0, field 0
    kept_seed = next(s for s, f in first.items() if f >= thr)
    dropped_seed = next(s for s, f in first.items() if f < thr)
    for seed, factor in ((kept_seed, 2.0), (dropped_seed, 0.0)):
        tr: dict = {}
        u = spec_tower_dropout(w, [[0, 3, 9]], sd, heads=1, act="gelu", mode="mean", n_i=True, n_u=True, max_history=8, p_hidden=0.0,
                               p_attn=p_attn, seed=seed, call=0, trace=tr)
        assert tr["attn_keep"][0].tolist() == [[[factor > 0]]]
        assert torch.equal(tr["ctx"][0], factor * tr["v"][0]) and float(tr["v"][0].abs().max()) > 0
        assert bool(torch.isfinite(u).all())
    assert float(scale_of(thr, torch.float64)) == 2.0 and float(scale_of(threshold(0.9375), torch.float32)) == 16.0  # noqa: PLR2004


def test_config_validation(mf):
    C = mf.models.ModelConfig
    cfg = C()
    assert (cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob, cfg.dropout_seed) == (0.0, 0.0, 0)
    cfg = C(user_tower="transformer", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.25, dropout_seed=7)
    assert (cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob, cfg.dropout_seed) == (0.1, 0.25, 7)
    for name in ("hidden_dropout_prob", "attention_probs_dropout_prob"):
        for bad in (1.0, -0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match=name):
                C(user_tower="transformer", **{name: bad})
        assert getattr(C(user_tower="transformer", **{name: 0.999}), name) == 0.999  # noqa: PLR2004
        for other in ("table", "history", "features"):
            with pytest.raises(ValueError, match="transformer"):
                C(user_tower=other, **{name: 0.1})
            assert getattr(C(user_tower=other, **{name: 0.0}), name) == 0.0
    with pytest.raises(ValueError, match="dropout_seed"):
        C(user_tower="transformer", dropout_seed=-1)
    lit = mf.lightning.MatrixFactorizationLitConfig(user_tower="transformer", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    assert mf.lightning.MatrixFactorizationLitConfig.model_validate(lit.model_dump()) == lit
    item = mf.models.EmbeddingTower(10, 32)
    for kw in ({"hidden_dropout_prob": 1.0}, {"attention_probs_dropout_prob": -0.5}, {"dropout_seed": 1 << 64}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            mf.models.HistoryTransformerTower(item, **kw)


def test_tower_surface(mf):
    towers = mf.models.init_towers(mf.models.ModelConfig(num_items=40, hidden_size=32, user_tower="transformer", hidden_dropout_prob=0.1,
                                                         attention_probs_dropout_prob=0.2, dropout_seed=5))
    plain = mf.models.init_towers(mf.models.ModelConfig(num_items=40, hidden_size=32, user_tower="transformer"))
    user = towers["user"]
    assert (user.hidden_dropout_prob, user.attention_probs_dropout_prob, user.dropout_seed, user.dropout_call) == (0.1, 0.2, 5, 0)
    assert (plain["user"].hidden_dropout_prob, plain["user"].attention_probs_dropout_prob) == (0.0, 0.0)
    assert list(user.state_dict()) == list(plain["user"].state_dict())         # seed and counter are not saved
    assert list(towers.state_dict()) == list(plain.state_dict())
    user.dropout_call = 9
    assert user.manual_seed(77) is user and (user.dropout_seed, user.dropout_call) == (77, 0)
    assert "0.1 / 0.1" in type(user).__doc__ and "hidden_dropout_prob=0.1" in repr(user)


def test_exports_are_bound_and_refuse_bad_probabilities(mf):
    lib = mf._lib.lib()
    header = (mf._lib._PKG.parent / "include" / "mf_hip.h").read_text()
    for name in ("mf_xfmr_forward_dropout", "mf_xfmr_backward_dropout", "mf_xfmr_backward_dropout_ws_bytes", "mf_dropout_words"):
        assert name in mf._lib.SIGNATURES and f"{name}(" in header and getattr(lib, name) is not None
    assert lib.mf_xfmr_backward_dropout_ws_bytes(100, 32, 64) == lib.mf_xfmr_backward_ws_bytes(100, 32, 64) + 100 * 32 * 4
    # the weight gradients' 256 split-K partials fit the workspace also when the intermediate size is below the hidden size
    # (the [h, h] + h partials of the attention weights are then the largest; the dropout's masked copy sits behind them)
    for h, inter in ((128, 32), (128, 96), (64, 32), (32, 128)):
        need = 256 * (max(h, inter) * h + max(h, inter)) * 4
        assert lib.mf_xfmr_backward_ws_bytes(8, h, inter) >= need + 7 * 8 * h * 4, (h, inter)
    # the probabilities are checked before anything else: no pointer is read, no GPU call is made
    fwd = (None, 10, 32, None, None, None, 1, 1, 1, 8, 1, 4, 32, 0, 0, 1, 1, None, None, None, None, None, 0)
    bwd = (32, 1, 1, 8, 8, 1, 4, 32, 0, 0, 1, None, None, None, None, None, None, None, None, None, 0)
    for ph, pa in ((1.0, 0.0), (0.0, 1.0), (-0.25, 0.1), (0.1, float("nan"))):
        assert lib.mf_xfmr_forward_dropout(*fwd, ph, pa, 0, 0, None) == mf._lib.MF_EINVAL
        assert b"[0, 1)" in lib.mf_last_error()
        assert lib.mf_xfmr_backward_dropout(*bwd, ph, pa, 0, 0, None) == mf._lib.MF_EINVAL
    assert ctypes.sizeof(ctypes.c_uint64) == 8  # noqa: PLR2004
