"""GPU: the bf16-mixed precision of the transformer user tower's dense layers (*Mixed precision*).

1 - 3 hold the GEMM engine to its arithmetic contract directly, through ``mf_xfmr_dense`` (one dense operation on caller
buffers, the tower's own launches): exactly on a lattice where every partial sum is exact, exactly on round-to-nearest-even
ties, and within the fp32 summation bound on normal operands.  4 - 8 hold the tower (``precision="bf16-mixed"``) to the mixed
spec of tests/test_xfmr_mixed_cpu.py in fp64, under that file's tolerance rule (8 E + 1e-7, E the largest fp32-spec error over
the eight worlds of a shape; rehearsed there on the CPU), and check reproducibility and serving.  Every figure is printed before
it is asserted (``pytest -s``)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests.test_gpu_xfmr_tower import DEV, _padded, _segments, _world, _zipf_lists
from tests.test_xfmr_mixed_cpu import (DROPOUT, DROPOUT_CASE, LR, SEEDS, TOWER_CASES, flatten, hold, reference, rel_err, round_bf16,
                                       tower_world, trunc_bf16)

pytestmark = pytest.mark.gpu
FP32, MIXED = 0, 1
WORST: dict = {}                 # tensor family -> the largest kernel error / E seen (printed by the tower tests)


# ---------------------------------------------------------------------------------- mf_xfmr_dense ----
def dense(mf, form: int, precision: int, a: torch.Tensor, b: torch.Tensor, bias: torch.Tensor | None = None):
    """form 0: (Y [M, N],) from a = X [M, K], b = W [N, K]; form 1: (dX [M, K],) from a = dY [M, N], b = W [N, K];
    form 2: (dW [N, K], db [N]) from a = dY [M, N], b = X [M, K].  CPU fp32 tensors in, CPU fp32 tensors out."""
    lib = mf._lib.lib()
    M = a.shape[0]
    N, K = (b.shape if form < 2 else (a.shape[1], b.shape[1]))  # noqa: PLR2004
    ad, bd = a.float().contiguous().to(DEV), b.float().contiguous().to(DEV)
    biasd = bias.float().contiguous().to(DEV) if bias is not None else None
    out = torch.full({0: (M, N), 1: (M, K), 2: (N, K)}[form], float("nan"), device=DEV)
    out_bias = torch.full((N,), float("nan"), device=DEV) if form == 2 else None  # noqa: PLR2004
    ws = mf._lib.workspace(lib.mf_xfmr_dense_ws_bytes(form, N, K), DEV)
    mf._lib.check(lib.mf_xfmr_dense(form, precision, M, N, K, ad.data_ptr(), bd.data_ptr(), mf._lib.ptr(biasd), out.data_ptr(),
                                    mf._lib.ptr(out_bias), ws.data_ptr(), ws.numel(), mf._lib.stream_ptr()))
    return (out.cpu(),) if out_bias is None else (out.cpu(), out_bias.cpu())


def dense_ref(form: int, a: torch.Tensor, b: torch.Tensor, bias: torch.Tensor | None = None):
    """The same in fp64 (exact on the lattices below)."""
    a, b = a.double(), b.double()
    if form == 0:
        return (a @ b.t() + (bias.double() if bias is not None else 0.0),)
    if form == 1:
        return (a @ b,)
    return a.t() @ b, a.sum(0)


def lattice(g: torch.Generator, *shape) -> torch.Tensor:
    """{-4 .. 4} / 8: exact in bf16; products are multiples of 1/64 below 1/4 and every fp32 partial sum of 1000 is exact."""
    return torch.randint(-4, 5, shape, generator=g).float() / 8


TOKENS = (1, 15, 16, 17, 63, 64, 65, 257, 1000)     # tails of the 16-deep k step (form 2) and of the 64-row tile (forms 0, 1)
WIDTHS = [(32, 32), (64, 128), (96, 64), (512, 128), (128, 512), (128, 96)]   # ragged 64-column tiles (32, 96), I < h, the widest


@pytest.mark.parametrize(("N", "K"), WIDTHS)
def test_engine_is_exact_on_a_lattice(mf, N, K):
    """1. All three forms, both precisions: ``torch.equal`` to the fp64 value (the lattice is exact in fp32 too)."""
    g = torch.Generator().manual_seed(N + K)
    for M in TOKENS:
        x, dy, w, bias = lattice(g, M, K), lattice(g, M, N), lattice(g, N, K), lattice(g, N)
        for form, args in ((0, (x, w, bias)), (0, (x, w, None)), (1, (dy, w)), (2, (dy, x))):
            want = dense_ref(form, *args)
            for precision in (MIXED, FP32):
                got = dense(mf, form, precision, *args)
                for o, r in zip(got, want):
                    assert torch.equal(o.double(), r), (form, precision, M, N, K)


def test_rounding_is_to_nearest_even(mf):
    """2. Operands made of the ties 1 + 2^-8 (-> 1) and 1 + 3 2^-8 (-> 1 + 2^-6) times powers of two, one product per output:
    the outputs are the products of the RNE-rounded values, not of the truncated or the unrounded ones; db is unrounded."""
    g = torch.Generator().manual_seed(2)
    n = 32

    def ties(*shape):
        t = torch.where(torch.rand(shape, generator=g) < 0.5, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8)  # noqa: PLR2004
        sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)  # noqa: PLR2004
        return (t * sign * 2.0 ** torch.randint(-6, 7, shape, generator=g)).float()

    one_per_row = torch.zeros(n, n)
    one_per_row[torch.arange(n), torch.randperm(n, generator=g)] = ties(n)   # (one per column too: form 2 sums over rows)
    full = ties(n, n)

    def views(t):
        return (torch.from_numpy(f(t.numpy())) for f in (round_bf16, trunc_bf16, lambda v: v))

    for form in (0, 1, 2):
        got = dense(mf, form, MIXED, one_per_row, full)
        (rne, _), (cut, _), (raw, raw_sum) = ((*dense_ref(form, a, b), None)[:2] for a, b in zip(views(one_per_row), views(full)))
        assert torch.equal(got[0].double(), rne), form
        assert float((rne != cut).double().mean()) > 0.25 and float((rne != raw).double().mean()) > 0.5, form  # noqa: PLR2004
        assert not torch.equal(got[0].double(), cut) and not torch.equal(got[0].double(), raw), form
        if form == 2:  # noqa: PLR2004
            assert torch.equal(got[1].double(), raw_sum)
            assert not torch.equal(raw_sum, torch.from_numpy(round_bf16(one_per_row.numpy())).double().sum(0))
        assert torch.equal(dense(mf, form, FP32, one_per_row, full)[0].double(), raw), form


@pytest.mark.parametrize(("form", "M", "depth"), [(0, 257, 512), (1, 257, 128), (2, 1000, 1000)])
def test_normal_operands_within_the_summation_bound(mf, form, M, depth):
    """3. |got - fp64(rnd(A) rnd(B))| <= depth 2^-24 sum |rnd a| |rnd b| elementwise: the products of bf16 values are exact in
    fp32, so what is left is the rounding of `depth` fp32 additions in whatever order, each at most 2^-24 relative to a
    partial sum that the sum of the absolute products bounds (first-order; a bound derived, not measured)."""
    N, K = 128, 512
    g = torch.Generator().manual_seed(form)
    x, dy, w = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g), torch.randn(N, K, generator=g)
    a, b = {0: (x, w), 1: (dy, w), 2: (dy, x)}[form]
    assert depth == {0: K, 1: N, 2: M}[form]
    ar, br = (torch.from_numpy(round_bf16(t.numpy())) for t in (a, b))
    got = dense(mf, form, MIXED, a, b)
    want = dense_ref(form, ar, br)
    bound = depth * 2.0 ** -24 * dense_ref(form, ar.abs(), br.abs())[0]
    err = (got[0].double() - want[0]).abs()
    print(f"  form {form}: largest error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert float((got[0].double() - dense_ref(form, a, b)[0]).abs().max()) > 1e-3      # noqa: PLR2004  (the operands were rounded)
    if form == 2:  # noqa: PLR2004
        db_bound = depth * 2.0 ** -24 * a.double().abs().sum(0)
        assert bool(((got[1].double() - a.double().sum(0)).abs() <= db_bound).all())


# ------------------------------------------------------------------------------------------ the tower ----
def _towers(mf, w, sd, kw, *, dropout=None, **tower_kw):
    rows, h = w.shape
    item = mf.models.EmbeddingTower(rows, h, normalize=kw["n_i"], device=DEV)
    with torch.no_grad():
        item.weight.copy_(w.float())
    if dropout is not None:
        tower_kw.update(hidden_dropout_prob=dropout["p_hidden"], attention_probs_dropout_prob=dropout["p_attn"], dropout_seed=dropout["seed"])
    user = mf.models.HistoryTransformerTower(item, num_hidden_layers=sum(k.endswith("attention.self.query.weight") for k in sd),
                                             num_attention_heads=kw["heads"], hidden_act=kw["act"], pooling_mode=kw["mode"],
                                             intermediate_size=sd["encoder.layer.0.intermediate.dense.weight"].shape[0],
                                             max_position_embeddings=sd["embeddings.position_embeddings.weight"].shape[0],
                                             max_history=kw["max_history"], normalize=kw["n_u"], **tower_kw)
    user.load_state_dict({k: v.float() for k, v in sd.items()})
    return item, user


def _kernel_step(mf, case, seed, *, dropout=None):
    """One SGD step of the mixed tower on world `seed` of `case`: {tensor name: tensor}; segments on even seeds, padded on odd."""
    w, sd, lists, c, extra, kw = tower_world(case, seed)
    item, user = _towers(mf, w, sd, kw, dropout=dropout, precision="bf16-mixed")
    u = user(_padded(lists) if seed % 2 else _segments(lists))
    ids, c2 = extra
    loss = (u * c.float().to(DEV)).sum() + (item(ids.to(DEV)) * c2.float().to(DEV)).sum()
    loss.backward()
    before = item.weight.detach().clone()
    mf.optim.SparseSGD([item.weight], lr=LR).step()
    assert torch.equal(u[-1].detach().cpu(), torch.zeros(w.shape[1]))       # the empty list: exactly 0
    return flatten((u.detach(), item.weight.detach() - before, {k: p.grad for k, p in user.named_parameters()}))


def _hold_case(mf, case, dropout):
    ref64, e = reference(case, dropout is not None)
    for s in SEEDS:
        hold(f"{case} seed {s}", _kernel_step(mf, case, s, dropout=dropout), ref64[s], e, WORST)
    print("  largest kernel error / E so far:", {k: round(v, 2) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("case", TOWER_CASES, ids=lambda c: "-".join(map(str, c)))
def test_tower_forward_and_one_sgd_step(mf, case):
    """4. u, the table delta and every dense gradient against the fp64 mixed spec, on the eight worlds of the shape."""
    _hold_case(mf, case, None)


def test_really_bf16(mf):
    """5. The mixed tower's u is not the fp32 tower's; precision="fp32" is the tower built without the keyword, bit for bit."""
    w, sd, lists, c, extra, kw = tower_world(TOWER_CASES[1], 0)
    hist = _segments(lists)
    out = {}
    for name, tower_kw in (("default", {}), ("fp32", {"precision": "fp32"}), ("mixed", {"precision": "bf16-mixed"})):
        item, user = _towers(mf, w, sd, kw, **tower_kw)
        u = user(hist)
        (u * c.float().to(DEV)).sum().backward()
        out[name] = [u.detach()] + [p.grad for p in user.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(out["default"], out["fp32"]))
    moved = rel_err(out["mixed"][0].cpu(), out["fp32"][0].cpu())
    print(f"  bf16-mixed moves u by {moved:.3e}")
    assert moved > 1e-5                                                      # noqa: PLR2004


def test_tower_with_dropout(mf):
    """6. hidden / attention dropout 0.1 / 0.1 under manual_seed: the dropout spec with the rounding hook, same rule."""
    _hold_case(mf, DROPOUT_CASE, DROPOUT)


@pytest.mark.parametrize("dropout", [None, {"p_hidden": 0.1, "p_attn": 0.1, "seed": 9}], ids=["plain", "dropout"])
def test_two_adam_steps_are_bit_reproducible(mf, dropout):
    """7. No float atomics in the bf16 engine either: two runs from the same state are equal, tables and dense weights."""
    rng = np.random.default_rng(5)
    rows, d, L = 500, 64, 32
    w, sd = _world(11, rows, d, 2, 128, 64)
    lists = _zipf_lists(rng, rows, 512, 24)
    g = torch.Generator().manual_seed(5)
    c, ids, c2 = torch.randn(len(lists), d, generator=g), torch.randint(1, rows, (700,), generator=g), torch.randn(700, d, generator=g)
    kw = {"heads": 4, "act": "gelu", "mode": "max", "max_history": L, "n_i": True, "n_u": True}
    results = []
    for _ in range(2):
        item, user = _towers(mf, w, sd, kw, dropout=dropout, precision="bf16-mixed")
        opt = mf.optim.tower_optimizer(torch.nn.ModuleDict({"user": user, "item": item}), "adam", 0.01)
        assert isinstance(opt, mf.optim.TowerOptimizer)
        for step in range(2):
            hist = _segments(lists) if step == 0 else _padded([x[-L:] for x in lists])
            ((user(hist) * c.to(DEV)).sum() + (item(ids.to(DEV)) * c2.to(DEV)).sum()).backward()
            opt.step()
            opt.zero_grad()
        results.append([item.weight.detach().clone()] + [p.detach().clone() for p in user.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*results))
    assert not torch.equal(results[0][0].cpu(), w.float())
    moved = [not torch.equal(a.cpu(), sd[k].float()) for a, k in zip(results[0][1:], dict(user.named_parameters()))]
    assert sum(moved) >= len(moved) - 1                # every dense weight stepped (token-type row 1 has no gradient)


def test_eval_mode_serving(mf):
    """8. ``recommend`` on a module built with precision="bf16-mixed" serves the mixed tower's own u (no switching)."""
    m = mf.lightning.MatrixFactorizationLitModule({"num_users": 40, "num_items": 300, "hidden_size": 64, "user_tower": "transformer",
                                                   "max_history": 16, "num_hidden_layers": 2, "precision": "bf16-mixed"})
    m.configure_model(device=DEV)
    user, item = m.towers["user"], m.towers["item"]
    assert user.precision == "bf16-mixed" and "precision=bf16-mixed" in repr(user)
    with torch.no_grad():                              # BERT's 0.02 initialisation barely moves u: widen the dense weights
        for p in user.parameters():
            p.mul_(8.0)
    index = m.item_processor.get_index(m)
    rng = np.random.default_rng(8)
    m.history = {b: rng.integers(1, 300, n).tolist() for b, n in ((3, 1), (5, 9), (7, 16), (11, 40))}
    fp32 = mf.models.HistoryTransformerTower(item, num_hidden_layers=2, max_history=16).eval()
    fp32.load_state_dict(user.state_dict())
    for b, hist in m.history.items():
        rec = m.recommend(b, top_k=10)
        assert user.training and user.precision == "bf16-mixed"
        with torch.no_grad():
            u = user.eval()(torch.tensor([hist], device=DEV))
            user.train()
            _, rows = index.search(u, 10, exclude=[sorted(set(hist))])
            moved = rel_err(u.cpu(), fp32(torch.tensor([hist], device=DEV)).cpu())
        assert rec["movie_rn"].tolist() == rows[0].cpu().tolist(), b
        assert moved > 1e-5, (b, moved)                                      # noqa: PLR2004
