"""CPU: the spec of the transformer user tower (``spec_tower``, plain torch -- the GPU tests hold the kernels to it, and it is
held here to ``transformers.BertModel`` and to the fixture ``tests/golden/xfmr_*.npz``), the configuration surface, the
parameter names, the combined optimiser and the new kernels' register budgets."""
from __future__ import annotations

import importlib.util
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import GOLDEN, ROOT

ACTS = {"gelu": F.gelu, "relu": F.relu, "silu": F.silu, "gelu_new": lambda x: F.gelu(x, approximate="tanh")}
FIXTURE = GOLDEN / "xfmr_h32_l1_a4_i32_L16.npz"


def spec_encoder(x: torch.Tensor, sd: dict, *, heads: int, act: str, prefix: str = "", trace: dict | None = None) -> torch.Tensor:
    """``[n, h]`` outputs of the BERT encoder (eval mode: no dropout) over the n valid rows ``x`` of ONE user, positions
    0 .. n - 1: e = LN((x + tok[0]) + pos[t]); per layer Q / K / V dense, ``heads`` heads, scores / sqrt(h / heads), softmax
    over the (valid) keys, context, dense + residual + LN; dense + act, dense + residual + LN.  LN eps 1e-12.  ``sd``:
    parameters under BertModel's ``state_dict`` names (after ``prefix``).  ``trace`` (a dict of lists) receives, detached, the
    rows entering every LayerNorm ("ln_in.<name>"), every layer's attention logits [heads, n, n] ("logits") and
    pre-activations [n, I] ("pre_act"): what the conditions of the hard worlds are computed from."""
    n, h = x.shape
    dh = h // heads

    def p(name):
        return sd[prefix + name]

    def note(key, v):
        if trace is not None:
            trace.setdefault(key, []).append(v.detach())
        return v

    def ln(v, name):
        return F.layer_norm(note("ln_in." + name, v), (h,), p(name + ".weight"), p(name + ".bias"), 1e-12)

    def dense(v, name):
        return F.linear(v, p(name + ".weight"), p(name + ".bias"))

    e = ln((x + p("embeddings.token_type_embeddings.weight")[0]) + p("embeddings.position_embeddings.weight")[:n], "embeddings.LayerNorm")
    layer = 0
    while f"{prefix}encoder.layer.{layer}.attention.self.query.weight" in sd:
        base = f"encoder.layer.{layer}."
        q, k, v = (dense(e, f"{base}attention.self.{name}").view(n, heads, dh).transpose(0, 1) for name in ("query", "key", "value"))
        prob = torch.softmax(note("logits", q @ k.transpose(-1, -2) / math.sqrt(dh)), dim=-1)
        ctx = (prob @ v).transpose(0, 1).reshape(n, h)
        y1 = ln(dense(ctx, f"{base}attention.output.dense") + e, f"{base}attention.output.LayerNorm")
        f = ACTS[act](note("pre_act", dense(y1, f"{base}intermediate.dense")))
        e = ln(dense(f, f"{base}output.dense") + y1, f"{base}output.LayerNorm")
        layer += 1
    return e


def spec_pool(y: torch.Tensor, mode: str, normalize: bool) -> torch.Tensor:
    """mean / channel-wise max (ties: the first position) / position 0 of the rows, then p / max(|p|, 1e-12)."""
    if mode == "mean":
        p = y.mean(0)
    elif mode == "cls":
        p = y[0]
    else:
        m = y.detach().max(0).values
        pos = torch.arange(y.shape[0])[:, None].expand_as(y)
        first = torch.where(y.detach() == m, pos, y.shape[0]).min(0).values
        p = y.gather(0, first[None]).squeeze(0)
    return F.normalize(p, dim=0, eps=1e-12) if normalize else p


def spec_tower(w: torch.Tensor, lists, sd: dict, *, heads: int, act: str, mode: str, n_i: bool, n_u: bool, max_history: int,
               prefix: str = "", trace: dict | None = None) -> torch.Tensor:
    """``[B, d]`` user vectors of the transformer tower, differentiable in ``w`` and ``sd``: ids outside [1, rows) are
    padding, the last ``max_history`` valid entries are kept (oldest at position 0), x = the (normalised) rows; an empty
    list gives 0."""
    rows, d = w.shape
    out = []
    for lst in lists:
        valid = [int(i) for i in lst if 1 <= int(i) < rows][-max_history:]
        if not valid:
            out.append(w.sum() * 0 + torch.zeros(d, dtype=w.dtype))
            continue
        x = w[torch.tensor(valid)]
        if n_i:
            x = F.normalize(x, dim=1, eps=1e-12)
        out.append(spec_pool(spec_encoder(x, sd, heads=heads, act=act, prefix=prefix, trace=trace), mode, n_u))
    return torch.stack(out)


def spec_trace(w: torch.Tensor, lists, sd: dict, **kw) -> dict:
    """The intermediate values of ``spec_tower`` on this batch (``spec_encoder``'s ``trace``), one list entry per user and layer."""
    trace: dict = {}
    with torch.no_grad():
        spec_tower(w, lists, sd, trace=trace, **kw)
    return trace


def spec_logits(w: torch.Tensor, lists, sd: dict, **kw) -> list:
    """Every (user, layer)'s attention logits ``[heads, n, n]`` (query, key), from the spec's own q and k."""
    return spec_trace(w, lists, sd, **kw)["logits"]


def random_state(g: torch.Generator, h: int, layers: int, inter: int, max_pos: int, *, std: float = 0.2, pos_std: float | None = None,
                 dtype=torch.float32) -> dict:
    """Encoder parameters under BertModel's names, drawn wide enough that every term matters (LN weights around 1)."""
    def rnd(*shape, s=std):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * s).to(dtype)

    sd = {"embeddings.position_embeddings.weight": rnd(max_pos, h, s=pos_std if pos_std is not None else std),
          "embeddings.token_type_embeddings.weight": rnd(2, h),
          "embeddings.LayerNorm.weight": 1 + rnd(h), "embeddings.LayerNorm.bias": rnd(h)}
    for i in range(layers):
        b = f"encoder.layer.{i}."
        for name in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
            sd[b + name + ".weight"], sd[b + name + ".bias"] = rnd(h, h), rnd(h)
        sd[b + "intermediate.dense.weight"], sd[b + "intermediate.dense.bias"] = rnd(inter, h), rnd(inter)
        sd[b + "output.dense.weight"], sd[b + "output.dense.bias"] = rnd(h, inter), rnd(h)
        for name in ("attention.output.LayerNorm", "output.LayerNorm"):
            sd[b + name + ".weight"], sd[b + name + ".bias"] = 1 + rnd(h), rnd(h)
    return sd


# ------------------------------------------------------------------------------------------ hard worlds ----
# Encoder states (plain state_dicts for spec_tower) that put the kernels where random_state(std=0.2) never does.  Every
# builder is seeded; the conditions that make a world mean something are asserted below from the fp64 spec alone
# (test_hard_world_conditions), and the GPU tests (tests/test_gpu_xfmr_tower.py) run the cases of HARD_CASES.
def sharp_state(g: torch.Generator, h: int, layers: int, inter: int, max_pos: int, *, heads: int, shift: float = 260.0,
                spread: float = 2.5) -> dict:
    """Attention nearly one-hot at logits in the hundreds: the query / key weights are scaled so that the logits of one
    query spread by about ``spread`` around their mean (the largest of 64 keys then leads the rest by several units:
    most of the mass on one key, a minority of the keys above 1e-6), and a common component in the query and key biases
    puts every logit near ``+shift``: exp(logit) overflows fp32 unless the row maximum is subtracted first."""
    sd = random_state(g, h, layers, inter, max_pos, dtype=torch.float64)
    dh = h // heads
    for i in range(layers):
        b = f"encoder.layer.{i}.attention.self."
        # rows entering a layer are LayerNorm outputs (entries ~ 1): q, k entries ~ 0.2 sqrt(h) s; logit spread ~ (0.2 sqrt(h) s)^2
        s = math.sqrt(spread) / (0.2 * math.sqrt(h))
        c = math.sqrt(shift / math.sqrt(dh))             # c * c * dh / sqrt(dh) = shift
        for name in ("query", "key"):
            sd[b + name + ".weight"] = sd[b + name + ".weight"] * s
            sd[b + name + ".bias"] = sd[b + name + ".bias"] * s + c
    return sd


def saturated_state(g: torch.Generator, h: int, layers: int, inter: int, max_pos: int, *, act: str) -> dict:
    """Pre-activations with a standard deviation of about 20 (both tails beyond +-10 well filled); for SiLU every eighth
    intermediate channel carries a bias of -110, so that exp(-x) is inf in fp32 there."""
    sd = random_state(g, h, layers, inter, max_pos, dtype=torch.float64)
    for i in range(layers):
        b = f"encoder.layer.{i}.intermediate.dense."
        s = 20.0 / (0.2 * math.sqrt(h))
        sd[b + "weight"] = sd[b + "weight"] * s
        sd[b + "bias"] = sd[b + "bias"] * s
        if act == "silu":
            sd[b + "bias"][::8] = -110.0
        o = f"encoder.layer.{i}.output.dense."
        sd[o + "weight"] = sd[o + "weight"] / 8.0             # act(a) ~ 10: keep z2 = f Wo2^T + y1 of the order of y1
    return sd


def offset_state(g: torch.Generator, h: int, layers: int, inter: int, max_pos: int, *, offset: float = 600.0) -> dict:
    """Rows entering every LayerNorm with |mean| >> std: token-type row 0 and the attention / output dense biases carry a
    common offset; the LayerNorm weights are 10^U(-1, 1) (two decades)."""
    sd = random_state(g, h, layers, inter, max_pos, dtype=torch.float64)
    sd["embeddings.token_type_embeddings.weight"][0] += offset / 40.0       # (the embedding rows spread by ~ 0.3)
    for k in sd:
        if k.endswith("LayerNorm.weight"):
            sd[k] = 10.0 ** (torch.rand(h, generator=g, dtype=torch.float64) * 2 - 1)
        if k.endswith("output.dense.bias"):                                    # attention.output.dense and output.dense
            sd[k] = sd[k] + offset
    return sd


FLAT_ITEMS = 12          # ids 1 .. 12 of a flat world: 1 .. 6 constant rows, 7 .. 12 nearly constant
FLAT_POSITIONS = 4       # positions 0 .. 3 carry zero position rows


def flat_world(g: torch.Generator, rows: int, h: int, layers: int, inter: int, max_pos: int):
    """(w, sd, lists): used with un-normalised item rows.  Items 1 .. 6 are the constant vector 0.5, items 7 .. 12 are
    0.5 +- 2^-10 (as many + as -), token-type row 0 is the constant 0.25 and the first four position rows are zero: a flat
    item at one of those positions enters the embedding LayerNorm with variance exactly 0 (rstd = 1e6, the eps alone) or
    2^-20.  All of these values, their sums and their means are exact in fp32 in any order of summation, so the fp32
    reference does not lose the row before the kernels see it.  ``lists``: users whose tokens are all flat, users who mix
    flat and ordinary tokens, flat items at positions with a position row (not flat there), an ordinary user, an empty one."""
    sd = random_state(g, h, layers, inter, max_pos, dtype=torch.float64)
    sd["embeddings.token_type_embeddings.weight"][0] = 0.25
    sd["embeddings.position_embeddings.weight"][:FLAT_POSITIONS] = 0.0
    w = torch.randn(rows, h, generator=g, dtype=torch.float64) / h ** 0.5
    w[1:7] = 0.5
    for i in range(7, 13):
        sign = torch.ones(h, dtype=torch.float64)
        sign[torch.randperm(h, generator=g)[: h // 2]] = -1.0
        w[i] = 0.5 + sign * 2.0 ** -10
    other = lambda n: torch.randint(FLAT_ITEMS + 1, rows, (n,), generator=g).tolist()  # noqa: E731
    lists = [[1, 2, 3], [7, 8], [4, 9, 5, 10], [6, 11] + other(20), [1, 7, 2, 8] + other(60), other(3) + [3, 12, 4], other(64), [5], []]
    return w, sd, lists


def hard_lists(g: torch.Generator, rows: int, L: int) -> list:
    """Lists that fill L (one behind padding and out-of-range ids, one exactly L, one longer), short ones and an empty one."""
    ids = lambda n: torch.randint(1, rows, (n,), generator=g).tolist()  # noqa: E731
    first = ids(L + 9)
    first[1], first[5], first[L] = 0, rows + 5, -3
    return [first, ids(L), ids(2), ids(1), ids(max(1, L // 4) + 1), ids(3)[:2] + [0], []]


# (world, h, heads, L, mode, layers, act, intermediate): sharp at every head width (8, 16, 32, 64: h = 128 and h = 64 for
# width 64), every activation on saturated, mean and max on every world (cls once), h = 64 and h = 128 on every world
HARD_CASES = [
    ("sharp", 64, 8, 64, "mean", 1, "gelu", 64), ("sharp", 64, 4, 64, "max", 2, "relu", 96), ("sharp", 64, 2, 64, "cls", 1, "silu", 64),
    ("sharp", 128, 2, 64, "mean", 1, "gelu_new", 128), ("sharp", 64, 1, 64, "max", 1, "gelu", 64), ("sharp", 128, 16, 64, "max", 1, "gelu", 64),
    ("saturated", 64, 4, 64, "mean", 1, "gelu", 128), ("saturated", 128, 4, 64, "max", 1, "silu", 256),
    ("saturated", 64, 2, 64, "max", 2, "relu", 64), ("saturated", 128, 8, 64, "mean", 1, "gelu_new", 128),
    ("saturated", 64, 8, 64, "mean", 2, "silu", 160),
    ("offset", 64, 4, 64, "mean", 2, "gelu", 64), ("offset", 128, 8, 64, "max", 1, "silu", 128),
    ("flat", 64, 4, 64, "max", 1, "gelu", 64), ("flat", 128, 4, 64, "mean", 2, "relu", 128),
]
HARD_ROWS = 200


def hard_case(world: str, h: int, heads: int, L: int, mode: str, layers: int, act: str, inter: int):
    """(w, sd, lists, c, kw) of one entry of HARD_CASES, all fp64: the loss of the case is sum(u . c)."""
    g = torch.Generator().manual_seed(1000 + 7 * h + heads + 3 * layers + len(world))
    if world == "flat":
        w, sd, lists = flat_world(g, HARD_ROWS, h, layers, inter, L)
    else:
        if world == "sharp":
            sd = sharp_state(g, h, layers, inter, L, heads=heads)
        elif world == "saturated":
            sd = saturated_state(g, h, layers, inter, L, act=act)
        else:
            sd = offset_state(g, h, layers, inter, L)
        w = torch.randn(HARD_ROWS, h, generator=g, dtype=torch.float64) / h ** 0.5
        lists = hard_lists(g, HARD_ROWS, L)
    c = torch.randn(len(lists), h, generator=g, dtype=torch.float64)
    kw = {"heads": heads, "act": act, "mode": mode, "n_i": world != "flat", "n_u": True, "max_history": L}
    return w, sd, lists, c, kw


def spec_step(w, sd, lists, c, kw, extra, lr, dtype):
    """(u, table delta of one SGD step, dense gradients) of sum(u . c) [+ sum(v . c2)] through the spec, in ``dtype``."""
    wl = w.to(dtype).clone().requires_grad_(True)
    leaf = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    u = spec_tower(wl, lists, leaf, **kw)
    loss = (u * c.to(dtype)).sum()
    if extra is not None:
        ids, c2 = extra
        v = wl[ids]
        loss = loss + ((F.normalize(v, dim=1, eps=1e-12) if kw["n_i"] else v) * c2.to(dtype)).sum()
    loss.backward()
    delta = (wl.detach() - lr * wl.grad) - wl.detach()
    return u.detach(), delta, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}


def rel_err(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """max-abs error over the max-abs of the fp64 value (the measure of the GPU file's ``_check``)."""
    ref = ref64.double()
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30) if ref.numel() else 0.0


def tie_world(rows: int = 20, h: int = 64, length: int = 9):
    """(w, sd, lists) for exact max-pool ties: one position row for all positions, a history that repeats item 5."""
    g = torch.Generator().manual_seed(77)
    sd = random_state(g, h, 1, 64, 16, dtype=torch.float64)
    sd["embeddings.position_embeddings.weight"][:] = sd["embeddings.position_embeddings.weight"][0].clone()
    w = torch.randn(rows, h, generator=g, dtype=torch.float64) / h ** 0.5
    return w, sd, [[5] * length, [3, 7, 3]]


def load_fixture():
    z = np.load(FIXTURE)
    cfg = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg.")}
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}
    grads = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("dw.")}
    return z, cfg, sd, grads


def fixture_scalar(z, sd, x, mode, dtype):
    """The fixture's scalar sum(u . c) through the spec; returns (u [B, h], scalar)."""
    mask = torch.from_numpy(z["mask"]).bool()
    c = torch.from_numpy(z["c"]).to(dtype)
    us = []
    for b in range(x.shape[0]):
        n = int(mask[b].sum())
        if n == 0:
            us.append(x.sum() * 0 + torch.zeros(x.shape[2], dtype=dtype))
        else:
            us.append(spec_pool(spec_encoder(x[b, :n], sd, heads=int(z["cfg.heads"]), act="gelu"), mode, True))
    u = torch.stack(us)
    return u, (u * c).sum()


def test_spec_against_the_fixture():
    z, cfg, sd, grads = load_fixture()
    assert (cfg["h"], cfg["layers"], cfg["heads"], cfg["inter"], cfg["L"], cfg["B"]) == (32, 1, 4, 32, 16, 8)
    lengths = torch.from_numpy(z["mask"]).sum(1).tolist()
    assert {0, 1, 9, 16} <= set(lengths)
    for mode in ("mean", "max", "cls"):
        x = torch.from_numpy(z["inputs_embeds"]).clone().requires_grad_(True)
        leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        u, s = fixture_scalar(z, leaf, x, mode, torch.float32)
        assert torch.allclose(u, torch.from_numpy(z[f"u.{mode}"]), atol=2e-6), mode
        if mode == "mean":
            s.backward()
            assert torch.allclose(x.grad, torch.from_numpy(z["d_inputs_embeds"]), atol=2e-6)
            for k, v in leaf.items():
                want = grads[k]
                got = v.grad if v.grad is not None else torch.zeros_like(v)
                assert torch.allclose(got, want, atol=1e-5 * max(1.0, float(want.abs().max()))), k


@pytest.mark.parametrize("act", sorted(ACTS))
def test_spec_against_bert_model(act):
    transformers = pytest.importorskip("transformers")
    from transformers.models.bert import BertConfig, BertModel

    del transformers
    g = torch.Generator().manual_seed(1)
    h, layers, heads, inter, L, B = 32, 2, 4, 64, 16, 5
    torch.manual_seed(0)
    model = BertModel(BertConfig(vocab_size=4, hidden_size=h, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=inter,
                                 hidden_act=act, max_position_embeddings=L), add_pooling_layer=False).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.1)
    sd = {k: v for k, v in model.state_dict().items() if "word_embeddings" not in k and v.dtype.is_floating_point}
    lengths = [1, 7, 16, 3, 12]
    x = torch.randn(B, L, h, generator=g)
    mask = torch.zeros(B, L, dtype=torch.int64)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    with torch.no_grad():
        want = model(inputs_embeds=x, attention_mask=mask).last_hidden_state
        for b, n in enumerate(lengths):
            got = spec_encoder(x[b, :n], sd, heads=heads, act=act)
            assert torch.allclose(got, want[b, :n], atol=5e-6), (b, float((got - want[b, :n]).abs().max()))


def _case_id(case) -> str:
    return "-".join(str(x) for x in case)


@pytest.mark.parametrize("case", HARD_CASES, ids=_case_id)
def test_hard_world_conditions(case):
    """What makes a hard world mean something, from the fp64 spec alone, for every case the GPU tests run on it.

    sharp: the largest logit is >= 200 (exp overflows fp32 without the max subtraction; the smallest is positive too, so
    every row needs it) and >= 10 % of the (query, key) pairs of users with n >= 2 are a non-maximal key with probability
    > 1e-6.  saturated: >= 10 % of the pre-activations above +10 and >= 10 % below -10; SiLU: >= 5 below -90.  offset: the
    median over tokens of |mean| / std of the rows entering each LayerNorm is >= 30.  flat: a token whose variance before
    the embedding LayerNorm is < 1e-10.

    Every world: the fp32 CPU spec is finite and within 1e-3 of the fp64 spec for u, the table step and every parameter
    gradient (max-abs over max-abs), so that the GPU tolerance, a multiple of that error, stays a real bound.  One tensor
    cannot be held to a relative cap: the key bias adds q . b_k to every logit of a query, which the softmax removes, so
    its gradient is exactly 0 and the fp64 value is rounding noise; it is held to 1e-3 of the query bias gradient's scale
    (same layer, same units) instead."""
    world = case[0]
    w, sd, lists, c, kw = hard_case(*case)
    tr = spec_trace(w, lists, sd, **kw)
    if world == "sharp":
        assert spec_logits(w, lists, sd, **kw)[0].shape[0] == kw["heads"]
        assert max(float(x.max()) for x in tr["logits"]) >= 200.0            # noqa: PLR2004
        assert min(float(x.min()) for x in tr["logits"]) > 100.0             # noqa: PLR2004
        pairs = alive = 0
        for x in tr["logits"]:
            if x.shape[-1] < 2:                                                # noqa: PLR2004
                continue
            prob = torch.softmax(x, -1)
            not_max = torch.ones_like(prob, dtype=torch.bool).scatter_(-1, x.argmax(-1, keepdim=True), False)
            pairs += prob.numel()
            alive += int(((prob > 1e-6) & not_max).sum())                      # noqa: PLR2004
        assert alive >= 0.1 * pairs, (alive, pairs)
    elif world == "saturated":
        a = torch.cat([x.flatten() for x in tr["pre_act"]])
        assert float((a > 10).float().mean()) >= 0.1 and float((a < -10).float().mean()) >= 0.1  # noqa: PLR2004
        if kw["act"] == "silu":
            assert int((a < -90).sum()) >= 5                                   # noqa: PLR2004
            assert not math.isfinite(float(torch.exp(-a.min().float())))       # exp(-x) is inf in fp32
    elif world == "offset":
        norms = [k for k in tr if k.startswith("ln_in.")]
        assert len(norms) == 1 + 2 * case[5]
        for k in norms:
            z = torch.cat(tr[k])
            assert float((z.mean(1).abs() / z.std(1, unbiased=False)).median()) >= 30.0, k  # noqa: PLR2004
        gammas = torch.cat([v for k, v in sd.items() if k.endswith("LayerNorm.weight")])
        assert float(gammas.max() / gammas.min()) >= 50.0                       # noqa: PLR2004
    else:
        var = torch.cat(tr["ln_in.embeddings.LayerNorm"]).var(1, unbiased=False)
        assert int((var < 1e-10).sum()) >= 1 and int(((var > 1e-10) & (var < 1e-5)).sum()) >= 1  # noqa: PLR2004
        assert all(bool((v.float().double() == v).all()) for v in (w[1: FLAT_ITEMS + 1], sd["embeddings.token_type_embeddings.weight"][0]))
    assert any(len([i for i in lst if 1 <= i < HARD_ROWS]) >= case[3] for lst in lists)          # a list fills L
    u64, d64, g64 = spec_step(w, sd, lists, c, kw, None, 0.5, torch.float64)
    u32, d32, g32 = spec_step(w, sd, lists, c, kw, None, 0.5, torch.float32)
    for name, got, ref in [("u", u32, u64), ("table step", d32, d64)] + [(k, g32[k], g64[k]) for k in g64]:
        assert bool(torch.isfinite(got).all()), name
        if name.endswith("attention.self.key.bias"):
            scale = float(g64[name.replace(".key.", ".query.")].abs().max())
            assert float(got.abs().max()) <= 1e-3 * scale and float(ref.abs().max()) <= 1e-3 * scale, name  # noqa: PLR2004
        else:
            assert rel_err(got, ref) <= 1e-3, (name, rel_err(got, ref))       # noqa: PLR2004


def test_max_pool_ties_spec_is_bit_identical_in_fp32_and_fp64():
    """The input of the GPU tie test: all position rows equal and a history that repeats ONE item, so that every token's
    row is the same at every depth of the encoder (attention over identical rows returns the row) and every channel of the
    max pool is an n-way tie.  The tie itself is exact in any precision: within one run of the spec all rows of the last
    layer are bit-identical, in fp64 and in fp32, so 'the first position wins' is well defined for the kernels too."""
    w, sd, lists = tie_world()
    for dtype in (torch.float64, torch.float32):
        tr: dict = {}
        x = F.normalize(w.to(dtype)[torch.tensor(lists[0])], dim=1, eps=1e-12)
        y = spec_encoder(x, {k: v.to(dtype) for k, v in sd.items()}, heads=4, act="gelu", trace=tr)
        assert all(torch.equal(y[0], y[j]) for j in range(1, y.shape[0])), dtype
        wl = w.to(dtype).clone().requires_grad_(True)
        spec_tower(wl, lists, {k: v.to(dtype) for k, v in sd.items()}, heads=4, act="gelu", mode="max", n_i=True, n_u=True,
                   max_history=16).sum().backward()
        assert float(wl.grad[lists[0][0]].abs().max()) > 0


def test_spec_hand_worked_single_token():
    """L = 1: attention is the identity on the one token (its softmax is 1), so ctx = V."""
    g = torch.Generator().manual_seed(2)
    h = 32
    sd = random_state(g, h, 1, 32, 4, dtype=torch.float64)
    w = torch.randn(6, h, generator=g, dtype=torch.float64)

    def ln(v, name):
        m, var = v.mean(), v.var(unbiased=False)
        return (v - m) / torch.sqrt(var + 1e-12) * sd[name + ".weight"] + sd[name + ".bias"]

    x = w[3] / w[3].norm()
    e = ln(x + sd["embeddings.token_type_embeddings.weight"][0] + sd["embeddings.position_embeddings.weight"][0], "embeddings.LayerNorm")
    b = "encoder.layer.0."
    v = sd[b + "attention.self.value.weight"] @ e + sd[b + "attention.self.value.bias"]
    y1 = ln(sd[b + "attention.output.dense.weight"] @ v + sd[b + "attention.output.dense.bias"] + e, b + "attention.output.LayerNorm")
    a = sd[b + "intermediate.dense.weight"] @ y1 + sd[b + "intermediate.dense.bias"]
    f = a * 0.5 * (1 + torch.erf(a / math.sqrt(2)))
    y2 = ln(sd[b + "output.dense.weight"] @ f + sd[b + "output.dense.bias"] + y1, b + "output.LayerNorm")
    for mode in ("mean", "max", "cls"):
        u = spec_tower(w, [[0, 3, 9], []], sd, heads=4, act="gelu", mode=mode, n_i=True, n_u=True, max_history=8)
        assert torch.allclose(u[0], y2 / y2.norm(), atol=1e-12) and torch.equal(u[1], torch.zeros(h, dtype=torch.float64))


def test_spec_depends_on_the_order_and_keeps_the_last_entries():
    g = torch.Generator().manual_seed(3)
    sd = random_state(g, 32, 1, 32, 8, pos_std=0.5)
    w = torch.randn(20, 32, generator=g)
    kw = {"heads": 4, "act": "gelu", "mode": "mean", "n_i": True, "n_u": True}
    a = spec_tower(w, [[1, 2, 3, 4]], sd, max_history=8, **kw)
    b = spec_tower(w, [[4, 3, 2, 1]], sd, max_history=8, **kw)
    assert float((a - b).abs().max()) > 1e-2
    cut = spec_tower(w, [[7, 0, 1, 2, 25, 3, 4]], sd, max_history=4, **kw)
    assert torch.equal(cut, a)


def test_config_validation(mf):
    C = mf.models.ModelConfig
    cfg = C(user_tower="transformer", pooling_mode="cls", hidden_size=64, num_attention_heads=8, max_history=20)
    assert (cfg.num_hidden_layers, cfg.intermediate_size, cfg.hidden_act, cfg.max_position_embeddings) == (1, None, "gelu", 64)
    # the three legacy refusals
    for mode in ("cls", "pooler"):
        with pytest.raises(ValueError, match="no transformer"):
            C(user_tower="history", pooling_mode=mode)
    with pytest.raises(ValueError, match="no transformer"):
        mf.models.HistoryPoolingTower(mf.models.EmbeddingTower(10, 32), pooling_mode="cls")
    with pytest.raises(ValueError, match="pooling_mode must be one of"):
        C(pooling_mode="sum")
    with pytest.raises(ValueError):
        C(user_tower="bert")
    # the limits of this tower
    bad = [({"pooling_mode": "pooler"}, "pooler"), ({"pooling_mode": "sum"}, "pooling_mode must be one of"),
           ({"hidden_size": 256}, "hidden_size"), ({"hidden_size": 48}, "hidden_size"),
           ({"num_attention_heads": 3}, "head width"), ({"hidden_size": 32, "num_attention_heads": 8}, "head width"),
           ({"hidden_size": 128, "num_attention_heads": 1}, "head width"),
           ({"intermediate_size": 48}, "intermediate_size"), ({"intermediate_size": 512}, "intermediate_size"),
           ({"num_hidden_layers": 0}, "num_hidden_layers"), ({"num_hidden_layers": 5}, "num_hidden_layers"),
           ({"hidden_act": "tanh"}, "hidden_act"), ({"max_position_embeddings": 65}, "max_position_embeddings"),
           ({"max_position_embeddings": 16, "max_history": 17}, "max_history"), ({"num_hashes": 2}, "plain item table"),
           ({"item_tower": "features"}, "plain item table")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            C(**{"user_tower": "transformer", "hidden_size": 64, **kw})
    assert C(user_tower="transformer", hidden_size=128, intermediate_size=512).intermediate_size == 512
    lit = mf.lightning.MatrixFactorizationLitConfig(user_tower="transformer", pooling_mode="cls", num_hidden_layers=2)
    assert mf.lightning.MatrixFactorizationLitConfig.model_validate(lit.model_dump()) == lit
    with pytest.raises(ValueError, match="EmbeddingTower"):
        mf.models.HistoryTransformerTower(mf.models.HashEmbeddingTower(100, 32))
    with pytest.raises(ValueError, match="table user towers only"):
        mf.distributed.ShardedTrainer(mf, "cpu", "adam", 0, num_users=4, num_items=4, dim=32, user_tower="transformer")


def test_parameter_names_and_shapes_mirror_bert_model(mf):
    h, inter, layers, max_pos = 64, 96, 2, 48
    towers = mf.models.init_towers(mf.models.ModelConfig(num_items=40, hidden_size=h, user_tower="transformer", num_hidden_layers=layers,
                                                         intermediate_size=inter, max_position_embeddings=max_pos, max_history=30))
    user, item = towers["user"], towers["item"]
    assert isinstance(user, mf.models.HistoryTransformerTower) and user.weight is item.weight and user.max_history == 30
    want = {"embeddings.position_embeddings.weight": (max_pos, h), "embeddings.token_type_embeddings.weight": (2, h),
            "embeddings.LayerNorm.weight": (h,), "embeddings.LayerNorm.bias": (h,)}
    for i in range(layers):
        b = f"encoder.layer.{i}."
        for name in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
            want[b + name + ".weight"], want[b + name + ".bias"] = (h, h), (h,)
        want[b + "intermediate.dense.weight"], want[b + "intermediate.dense.bias"] = (inter, h), (inter,)
        want[b + "output.dense.weight"], want[b + "output.dense.bias"] = (h, inter), (h,)
        for name in ("attention.output.LayerNorm", "output.LayerNorm"):
            want[b + name + ".weight"], want[b + name + ".bias"] = (h,), (h,)
    assert {k: tuple(v.shape) for k, v in user.state_dict().items()} == want
    assert len(user.encoder_parameters()) == 4 + 16 * layers == len(list(user.parameters()))
    assert sum(p is item.weight for p in towers.parameters()) == 1             # the table is optimised once
    assert "item.weight" in towers.state_dict() and "user.weight" not in towers.state_dict()
    transformers = pytest.importorskip("transformers")
    from transformers.models.bert import BertConfig, BertModel

    del transformers
    bert = BertModel(BertConfig(vocab_size=4, hidden_size=h, num_hidden_layers=layers, num_attention_heads=4, intermediate_size=inter,
                                max_position_embeddings=max_pos), add_pooling_layer=False)
    theirs = {k: tuple(v.shape) for k, v in bert.state_dict().items() if "word_embeddings" not in k and v.dtype.is_floating_point}
    assert theirs == want


def test_defaults_still_build_table_towers(mf):
    cfg = mf.models.ModelConfig(num_users=30, num_items=40, hidden_size=32)
    towers = mf.models.init_towers(cfg)
    assert type(towers["user"]) is mf.models.EmbeddingTower and len(list(towers.parameters())) == 2


def test_combined_optimizer_steps_a_table_and_a_dense_weight(mf, monkeypatch):
    """One ``step()`` drives the sparse row optimiser and ``torch.optim.AdamW``; the row update itself is a GPU kernel, so
    the sparse half is watched at its boundary here."""
    table = torch.nn.Parameter(torch.zeros(6, 32))
    dense = torch.nn.Parameter(torch.ones(4, 4))
    opt = mf.optim.TowerOptimizer(mf.optim.RowAdam([table], lr=0.5), torch.optim.AdamW([dense], lr=0.1, weight_decay=0.0))
    assert isinstance(opt, torch.optim.Optimizer) and [len(g["params"]) for g in opt.param_groups] == [1, 1]
    calls = []

    def fake_step(self, closure=None):
        calls.append("sparse")
        with torch.no_grad():
            table[2] -= 1.0

    monkeypatch.setattr(mf.optim.RowAdam, "step", fake_step)
    dense.grad = torch.ones(4, 4)
    opt.step()
    assert calls == ["sparse"] and float(table[2, 0]) == -1.0 and float(table[1, 0]) == 0.0
    assert torch.allclose(dense, torch.full((4, 4), 0.9), atol=1e-6)            # AdamW's first step moves by lr
    opt.zero_grad()
    assert dense.grad is None
    state = opt.state_dict()
    assert set(state) == {"sparse", "dense"} and state["dense"]["state"][0]["step"] == 1
    opt2 = mf.optim.TowerOptimizer(mf.optim.RowAdam([table], lr=0.5), torch.optim.AdamW([dense], lr=0.1))
    opt2.load_state_dict(state)
    assert opt2.dense.state_dict()["state"][0]["step"] == 1
    for g in opt.param_groups:
        g["lr"] = 0.25
    assert opt.sparse.param_groups[0]["lr"] == 0.25 and opt.dense.param_groups[0]["lr"] == 0.25   # one set of groups
    with pytest.raises(ValueError, match="towers"):
        mf.optim.tower_optimizer(torch.nn.ModuleDict(), "rmsprop", 0.1)


def test_module_builds_the_combined_optimizer(mf):
    module = mf.lightning.MatrixFactorizationLitModule({"user_tower": "transformer", "num_items": 50, "hidden_size": 32})
    module.configure_model()
    opt = module.configure_optimizers()
    assert isinstance(opt, mf.optim.TowerOptimizer) and isinstance(opt.sparse, mf.optim.RowAdam) and isinstance(opt.dense, torch.optim.AdamW)
    assert [p is module.towers["item"].weight for g in opt.sparse.param_groups for p in g["params"]] == [True]
    assert len([p for g in opt.dense.param_groups for p in g["params"]]) == 20
    plain = mf.lightning.MatrixFactorizationLitModule({"num_items": 50, "num_users": 20})
    plain.configure_model()
    assert type(plain.configure_optimizers()) is mf.optim.RowAdam


def test_exports_are_bound_and_built(mf):
    import ctypes

    names = ("mf_xfmr_ws_bytes", "mf_xfmr_forward", "mf_xfmr_backward_ws_bytes", "mf_xfmr_backward", "mf_xfmr_coalesce_ws_bytes",
             "mf_xfmr_coalesce")
    header = (ROOT / "include" / "mf_hip.h").read_text()
    handle = ctypes.CDLL(str(mf._lib.LIB_PATH))
    for name in names:
        assert name in mf._lib.SIGNATURES and f"{name}(" in header
        assert getattr(handle, name) is not None
    handle.mf_xfmr_ws_bytes.restype, handle.mf_xfmr_ws_bytes.argtypes = mf._lib.SIGNATURES["mf_xfmr_ws_bytes"]
    small, large = handle.mf_xfmr_ws_bytes(8, 100, 32, 1, 32), handle.mf_xfmr_ws_bytes(8, 100, 32, 2, 32)
    assert 0 < small < large


def test_xfmr_kernels_do_not_spill(mf):
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = kr.kernel_resources()
    mine = {k: v for k, v in res.items() if "xfmr_" in k or "XfmrEntries" in k or "list_cut_kernel" in k}   # (the cut is shared: mf_lists.h)
    assert len(mine) >= 35, sorted(mine)  # noqa: PLR2004
    for k, v in mine.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, k
        assert v["private_segment_fixed_size"] == 0, k
