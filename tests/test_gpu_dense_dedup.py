"""GPU: the distinct-column sweeps of the dense loss (csrc/mf_loss_cols.h) against oracle.losses.loss in float64.

Inputs are built as ``table[item_idx]`` / ``logq_table[item_idx]``, so copies are REAL copies.  Every case first asserts
that the call was served by the distinct-column path (``mf_loss_cols_info``) and that the device's N' equals the count the
copy rule gives on the CPU -- a silent return to the uncompacted sweeps fails the test.  Mode 2 (serve wherever possible) is
forced and restored by a fixture; the bars are those of tests/_dense_cases.py."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests import _dense_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
INFONCE = "InfomationNoiseContrastiveEstimationLoss"


@pytest.fixture(autouse=True)
def _few_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


@pytest.fixture()
def dedup_always(mf):
    lib = mf._lib.lib()
    lib.mf_set_dense_dedup(2)
    yield lib
    lib.mf_set_dense_dedup(1)


# ------------------------------------------------------------------------------------- cases ---
def _ids(name, b, n, g):
    if name == "few":                       # 300 values: N' <= 300, a few tiles, a ragged last one
        return torch.randint(1, 301, (n,), generator=g)
    if name == "one":                       # N' = 1, weight N, every column masked for every user
        return torch.full((n,), 7, dtype=torch.int64)
    if name == "heavy":                     # one id on ~700 columns, the rest distinct; users share positives
        ids = torch.arange(10, 10 + n)
        ids[torch.randperm(n, generator=g)[:700]] = 5
        ids[: b // 2] = ids[b // 2: 2 * (b // 2)].clone()[torch.randperm(b // 2, generator=g)]      # negatives equal to positives
        return ids
    if name == "half":                      # N / 2 values (as tests/_dense_cases.py)
        return torch.randint(1, n // 2 + 1, (n,), generator=g)
    if name.startswith("exact"):            # exactly k distinct values, every one present
        k = int(name[5:])
        ids = torch.randint(1, k + 1, (n,), generator=g)
        ids[torch.randperm(n, generator=g)[:k]] = torch.arange(1, k + 1)
        return ids
    raise AssertionError(name)


def build_case(family, name, b, n, seed):
    """rows and logQ looked up by id; ``name`` "half" with false copies: see below"""
    g = torch.Generator().manual_seed(seed)
    ids = _ids(name.split("+")[0], b, n, g)
    rows = int(ids.max()) + 1
    if family == "random":
        table = torch.nn.functional.normalize(torch.randn(rows, D, generator=g), dim=-1)
        u = torch.nn.functional.normalize(torch.randn(b, D, generator=g), dim=-1)
        logq_table = torch.log(torch.rand(rows, generator=g) * 0.9 + 0.05)
    else:
        s = dc.lattice_shift(D)
        table = torch.randint(-2, 3, (rows, D), generator=g).float() * 2.0 ** -s
        u = torch.randint(-2, 3, (b, D), generator=g).float() * 2.0 ** -s
        logq_table = None
    t = {"u": u, "v": table[ids].contiguous(), "item_idx": ids, "target": torch.randint(-2, 6, (b,), generator=g),
         "pos_idx": torch.randint(0, rows, (b, dc.P), generator=g),
         "logq": None if logq_table is None else logq_table[ids].contiguous()}
    t["pos_idx"][:, 0] = ids[:b]
    if name.endswith("+false"):
        # false copies: half the duplicate columns get fresh rows, a few keep their row and get another logQ (random family)
        first = {}
        dup = [j for j, i in enumerate(ids.tolist()) if first.setdefault(i, j) != j]
        pick = torch.tensor(dup)[torch.randperm(len(dup), generator=g)]
        fresh, lq_only = pick[: len(dup) // 2], pick[len(dup) // 2: len(dup) // 2 + 40]
        if family == "random":
            t["v"][fresh] = torch.nn.functional.normalize(torch.randn(len(fresh), D, generator=g), dim=-1)
            t["logq"][lq_only] = t["logq"][lq_only] - 0.125
        else:
            t["v"][fresh] = torch.randint(-2, 3, (len(fresh), D), generator=g).float() * 2.0 ** -dc.lattice_shift(D)
    if family == "random":
        t["sigma"], t["margin"] = 3.0, dict.fromkeys(ol.KINDS, 0.25)
    else:
        t["sigma"] = sigma = 2.0
        t["step"] = step = sigma * 2.0 ** -(2 * dc.lattice_shift(D) + 1)
        lg = ol.logits_fn(t["u"].double(), t["v"].double(), t["target"].double(), sigma)
        med = float(lg[t["target"] != 0].abs().median())
        t["margin"] = dict.fromkeys(ol.KINDS, round(med / step) * step + 0.5 * step)
        t["margin"].update(PairwiseHingeLoss=0.5 * step, PairwiseLogisticLoss=0.5 * step)
    return t


def distinct_columns(t):
    """N' by the copy rule: column j is a copy iff its id's first column f != j holds the same row bits and the same logQ bits"""
    ids = t["item_idx"].numpy()
    v = t["v"].numpy().view(np.int32)
    lq = (np.zeros(len(ids), np.float32) if t["logq"] is None else t["logq"].numpy()).view(np.int32)
    _, first_of, inv = np.unique(ids, return_index=True, return_inverse=True)
    f = first_of[inv]
    copy = (f != np.arange(len(ids))) & (v == v[f]).all(axis=1) & (lq == lq[f])
    return int((~copy).sum())


def cols_info(lib, ws):
    out = (ctypes.c_int64 * 9)()
    assert lib.mf_loss_cols_info(ws.data_ptr(), out) == 0, lib.mf_last_error()
    return dict(zip(("served", "ncols", "nt", "nsf", "tpsf", "nsu", "tpsu", "nsv", "tpsv"), list(out)))


def _to_dev(t):
    return {k: x.to(DEV) for k, x in t.items() if isinstance(x, torch.Tensor)}


def _loss_fn(mf, kind, t):
    return getattr(mf.losses, kind)(num_negatives=0, sigma=t["sigma"], margin=t["margin"][kind])


def _run_gpu(mf, kind, t, dev, info=None):
    u, v = dev["u"].clone().requires_grad_(), dev["v"].clone().requires_grad_()
    val = _loss_fn(mf, kind, t)(u, v, dev["target"], item_idx=dev["item_idx"], pos_idx=dev["pos_idx"], logq=dev.get("logq"))
    if info is not None:                                  # the workspace this forward used (kept by the autograd node)
        info.append(cols_info(mf._lib.lib(), val.grad_fn.saved_tensors[2]))
    val.backward()
    return val.detach(), u.grad, v.grad


CASES = {
    "1-few-ids": ("few", 1020, 4090),
    "2-one-id": ("one", 1020, 4090),
    "3-heavy-id-n-equals-b": ("heavy", 2990, 2990),
    "4-false-copies": ("half+false", 1500, 4400),
    "6-exactly-32": ("exact32", 300, 700),
    "6-exactly-33": ("exact33", 300, 700),
    "6-exactly-128": ("exact128", 300, 700),
}


def _check_case(mf, lib, name, b, n, make):
    p = {"tps_u": 1, "tps_v": 1, "nsplit_u": 0, "nsplit_v": 0}                 # (only names rows in a failure message)
    for family, kinds, grad_kinds in (("random", ol.KINDS, dc.SMOOTH), ("lattice", dc.HINGE, dc.HINGE)):
        t = make(family)
        want_cols = distinct_columns(t)
        dev = _to_dev(t)
        info = []
        got = {kind: _run_gpu(mf, kind, t, dev, info if kind != "AlignmentLoss" else None) for kind in kinds}
        for i in info:
            assert i["served"] == 1, (name, family, i)
            assert i["ncols"] == want_cols and i["nt"] == -(-want_cols // 128) * 4, (name, family, i, want_cols)
        want = dc.reference(t, kinds, grad_kinds)
        for kind in kinds:
            what = f"{name} {family} {kind} B={b} N={n} N'={want_cols}"
            val, du, dv = got[kind]
            dc.assert_value_close(float(val.cpu()), want[kind][0], t["sigma"], t["target"].numpy(), what)
            if kind in grad_kinds:
                dc.assert_grads_close_located(du.cpu().numpy(), want[kind][1], t["sigma"], what, "du", p)
                dc.assert_grads_close_located(dv.cpu().numpy(), want[kind][2], t["sigma"], what, "dv", p)
    return want_cols


@pytest.mark.parametrize("name", list(CASES))
def test_distinct_column_sweeps_match_float64_oracle(mf, dedup_always, name):
    ids, b, n = CASES[name]
    ncols = _check_case(mf, dedup_always, name, b, n, lambda family: build_case(family, ids, b, n, seed=len(name) + b + n))
    if ids == "few":
        assert ncols <= 300
    if ids == "one":
        assert ncols == 1
    if ids.startswith("exact"):
        assert ncols == int(ids[5:])
    if ids == "half+false":
        assert ncols > len(set(build_case("random", ids, b, n, seed=len(name) + b + n)["item_idx"].tolist()))    # false copies are kept


def test_unrelated_values_under_repeated_ids_are_all_kept(mf, dedup_always):
    """tests/_dense_cases.py draws v and logq per COLUMN under ids that repeat: no true copies, N' = N, and the device
    geometry is mf_loss_plan's"""
    b, n = 2000, 5190
    made = {"random": dc.random_case(b, n, D), "lattice": dc.lattice_case(b, n, D)}
    assert _check_case(mf, dedup_always, "5-no-copies", b, n, made.__getitem__) == n
    q = dc.plan(dedup_always, b, n, D)
    t, dev, info = made["random"], _to_dev(made["random"]), []
    _run_gpu(mf, INFONCE, t, dev, info)
    got = tuple(info[0][k] for k in ("nsf", "tpsf", "nsu", "tpsu", "nsv", "tpsv"))
    assert got == (q["nsplit_f"], q["tps_f"], q["nsplit_u"], q["tps_u"], q["nsplit_v"], q["tps_v"]), (info, q)


def test_distinct_column_sweeps_are_repeatable(mf, dedup_always):
    """the plan compacts in column order and counts with integer adds; the sweeps and the epilogue add in a fixed order: a
    second forward + backward gives the same bits, and so does a second backward on a retained graph"""
    ids, b, n = CASES["3-heavy-id-n-equals-b"]
    for kind, family in ((INFONCE, "random"), ("PairwiseHingeLoss", "lattice")):
        t = build_case(family, ids, b, n, seed=77)
        dev = _to_dev(t)
        info = []
        first = _run_gpu(mf, kind, t, dev, info)
        again = _run_gpu(mf, kind, t, dev, info)
        assert all(i["served"] == 1 and i["ncols"] == distinct_columns(t) for i in info), info
        for x, y, what in zip(first, again, ("loss", "du", "dv")):
            assert torch.equal(x, y), (kind, what, "second forward + backward")
        u, v = dev["u"].clone().requires_grad_(), dev["v"].clone().requires_grad_()
        val = _loss_fn(mf, kind, t)(u, v, dev["target"], item_idx=dev["item_idx"], pos_idx=dev["pos_idx"], logq=dev.get("logq"))
        val.backward(retain_graph=True)
        du1, dv1 = u.grad.clone(), v.grad.clone()
        u.grad = v.grad = None
        val.backward()
        assert torch.equal(val.detach(), first[0]) and torch.equal(du1, first[1]) and torch.equal(dv1, first[2]), kind
        assert torch.equal(u.grad, du1) and torch.equal(v.grad, dv1), (kind, "second backward on a retained graph")


def test_uncompacted_path_is_intact_after_the_distinct_column_one(mf):
    """mode 0 after mode 2 gives the bits of a mode-0 run before it"""
    lib = mf._lib.lib()
    ids, b, n = CASES["1-few-ids"]
    t = build_case("random", ids, b, n, seed=5)
    dev = _to_dev(t)
    try:
        lib.mf_set_dense_dedup(0)
        info = []
        fresh = _run_gpu(mf, INFONCE, t, dev, info)
        lib.mf_set_dense_dedup(2)
        served = _run_gpu(mf, INFONCE, t, dev, info)
        lib.mf_set_dense_dedup(0)
        after = _run_gpu(mf, INFONCE, t, dev, info)
    finally:
        lib.mf_set_dense_dedup(1)
    assert [i["served"] for i in info] == [0, 1, 0], info
    for x, y, what in zip(fresh, after, ("loss", "du", "dv")):
        assert torch.equal(x, y), what
    assert abs(float(served[0]) - float(fresh[0])) <= 1e-4 * max(1.0, abs(float(fresh[0])))


def test_captured_step_equals_the_eager_one(mf, dedup_always):
    """N' never reaches the host: a step replayed from a hipGraph -- on a batch with OTHER duplicates than the captured one --
    equals the eager step bit for bit"""
    g = torch.Generator().manual_seed(3)
    b, users, items = 256, 400, 300

    def batch():
        item = torch.cat([torch.randint(1, 40, (b,), generator=g), torch.randint(1, items, (b,), generator=g)])
        pos = torch.randint(0, items, (b, 4), generator=g)
        pos[:, 0] = item[:b]
        return {k: x.to(DEV) for k, x in dict(user=torch.randint(1, users, (b,), generator=g), item=item,
                                              target=torch.randint(1, 6, (b,), generator=g), pos=pos).items()}

    batches = [batch() for _ in range(3)]
    results = []
    for captured in (False, True):
        torch.manual_seed(0)
        towers = mf.models.init_towers(mf.models.ModelConfig(num_users=users, num_items=items, hidden_size=D), device=DEV)
        opt = mf.optim.SparseSGD(list(towers.parameters()), lr=0.05)
        fn = mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0)
        one = torch.ones((), device=DEV)

        def step(bt):
            loss = fn(towers["user"](bt["user"]), towers["item"](bt["item"]), bt["target"], item_idx=bt["item"], pos_idx=bt["pos"])
            loss.backward(one)
            opt.step()
            return loss.detach()

        if captured:
            run = mf.graph.CapturedStep(step, batches[0], optimizers=[opt], warmup=3)
        else:
            for _ in range(3):              # the capture's three warm-up steps are real steps on batch 0
                step(batches[0])
            run = step
        losses = [run(bt).clone() for bt in batches[1:]]
        results.append((losses, [p.detach().clone() for p in towers.parameters()]))
    (l0, p0), (l1, p1) = results
    assert all(torch.equal(x, y) for x, y in zip(l0, l1)), (l0, l1)
    assert all(torch.equal(x, y) for x, y in zip(p0, p1))
