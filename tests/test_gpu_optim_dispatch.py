"""GPU: which export a sparse row optimiser's ``step()`` reaches.  The five update exports of the loaded library are wrapped
to record and forward; tables are 8 rows x 32 (one case: x 64) with 4 parked ids each, one of them repeated.  Two pending
tables of one width, one parameter group (and, for Adam, one step count) are ONE pair call; anything else is one single call
per table, in parameter order; nothing pending is no call.  After every case the tables and their state equal, bit for bit,
copies stepped through the single-table exports directly."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = 8
SINGLE = {"sgd": "mf_update_sgd", "adagrad": "mf_update_adagrad", "adam": "mf_update_adam"}
PAIR = {"sgd": "mf_update_pair", "adagrad": "mf_update_pair_adagrad", "adam": "mf_update_pair"}
CLASS = {"sgd": "SparseSGD", "adagrad": "RowAdagrad", "adam": "RowAdam"}
STATE = {"sgd": (), "adagrad": ("sum",), "adam": ("exp_avg", "exp_avg_sq")}
HYPER = {"sgd": {"lr": 0.05, "weight_decay": 0.01}, "adagrad": {"lr": 0.05, "eps": 1e-6, "weight_decay": 0.01},
         "adam": {"lr": 0.01, "betas": (0.9, 0.99), "eps": 1e-6, "weight_decay": 0.01}}
KINDS = ("sgd", "adagrad", "adam")


@pytest.fixture
def calls(mf, monkeypatch):
    """[(export, first table's address)] of every update call, in order; the calls go through."""
    lib, seen = mf._lib.lib(), []
    first_table = {"mf_update_pair": 2, "mf_update_pair_adagrad": 1}             # (argument index; the single exports: 0)
    for name in {*SINGLE.values(), *PAIR.values()}:
        def wrapped(*args, _name=name, _real=getattr(lib, name)):
            seen.append((_name, args[first_table.get(_name, 0)]))
            return _real(*args)
        monkeypatch.setattr(lib, name, wrapped)
    return seen


def _tables(widths, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = []
    for k, d in enumerate(widths):
        p = torch.nn.Parameter(torch.randn(ROWS, d, generator=g).to(DEV))
        ids = torch.tensor([5, 2, 5, (3 + k) % ROWS], device=DEV)              # one id twice
        p._mf_pending = [(ids, torch.randn(4, d, generator=g).to(DEV), bool(k % 2))]
        params.append(p)
    return params


def _direct(mf, kind, p, state, pend, hyper, step):
    """One table through its single-table export, on copies: (table, {state name: tensor})."""
    lib, L = mf._lib.lib(), mf._lib
    ids, g, norm = pend
    w = p.detach().clone()
    st = {k: state[k].clone() for k in STATE[kind]}
    n, d = ids.numel(), w.shape[1]
    ws = L.workspace(lib.mf_update_ws_bytes(n, d), w.device)
    head = (w.data_ptr(), *(st[k].data_ptr() for k in STATE[kind]), ROWS, d, ids.data_ptr(), n, g.data_ptr(), int(norm))
    tail = (hyper["weight_decay"], ws.data_ptr(), ws.numel(), L.stream_ptr())
    if kind == "sgd":
        L.check(lib.mf_update_sgd(*head, hyper["lr"], *tail))
    elif kind == "adagrad":
        L.check(lib.mf_update_adagrad(*head, hyper["lr"], hyper["eps"], *tail))
    else:
        L.check(lib.mf_update_adam(*head, step, None, hyper["lr"], *hyper["betas"], hyper["eps"], *tail))
    return w, st


def _step_and_compare(mf, kind, opt, params, calls):
    """Step ``opt``; returns the recorded calls after comparing every table and its state with the direct path."""
    if kind != "sgd":
        opt.init_state()
    want = []
    for p in params:
        group = next(g for g in opt.param_groups if any(p is q for q in g["params"]))
        pend = p._mf_pending[0] if p._mf_pending else None
        if pend is not None:
            want.append(_direct(mf, kind, p, opt.state[p], pend, group, opt.state[p].get("step", 0) + 1))
        else:
            want.append((p.detach().clone(), {k: opt.state[p][k].clone() for k in STATE[kind]}))
    del calls[:]
    opt.step()
    torch.cuda.synchronize()
    for p, (w, st) in zip(params, want):
        assert torch.equal(p.detach(), w)
        for k in STATE[kind]:
            assert torch.equal(opt.state[p][k], st[k]), k
        assert not p._mf_pending                                                 # the parked rows are consumed
    return list(calls)


def _singles(kind, params):
    return [(SINGLE[kind], p.data_ptr()) for p in params]


@pytest.mark.parametrize("kind", KINDS)
def test_two_tables_of_one_group_are_one_pair_call(mf, calls, monkeypatch, kind):
    monkeypatch.delenv("MF_UPDATE_PAIR", raising=False)
    params = _tables([32, 32])
    opt = getattr(mf.optim, CLASS[kind])(params, **HYPER[kind])
    assert _step_and_compare(mf, kind, opt, params, calls) == [(PAIR[kind], params[0].data_ptr())]


@pytest.mark.parametrize("kind", KINDS)
def test_pair_switched_off_is_two_single_calls(mf, calls, monkeypatch, kind):
    monkeypatch.setenv("MF_UPDATE_PAIR", "0")
    params = _tables([32, 32], seed=1)
    opt = getattr(mf.optim, CLASS[kind])(params, **HYPER[kind])
    assert _step_and_compare(mf, kind, opt, params, calls) == _singles(kind, params)


def test_adam_tables_at_different_steps_are_two_single_calls(mf, calls, monkeypatch):
    monkeypatch.delenv("MF_UPDATE_PAIR", raising=False)
    params = _tables([32, 32], seed=2)
    opt = mf.optim.RowAdam(params, **HYPER["adam"])
    opt.init_state()
    opt.state[params[1]]["step"] = 3
    assert _step_and_compare(mf, "adam", opt, params, calls) == _singles("adam", params)
    assert [opt.state[p]["step"] for p in params] == [1, 4]


@pytest.mark.parametrize("kind", KINDS)
def test_two_parameter_groups_are_two_single_calls(mf, calls, monkeypatch, kind):
    monkeypatch.delenv("MF_UPDATE_PAIR", raising=False)
    params = _tables([32, 32], seed=3)
    opt = getattr(mf.optim, CLASS[kind])([{"params": [params[0]]}, {"params": [params[1]], "lr": 0.02}], **HYPER[kind])
    assert _step_and_compare(mf, kind, opt, params, calls) == _singles(kind, params)


@pytest.mark.parametrize("kind", KINDS)
def test_two_widths_are_two_single_calls(mf, calls, monkeypatch, kind):
    monkeypatch.delenv("MF_UPDATE_PAIR", raising=False)
    params = _tables([32, 64], seed=4)
    opt = getattr(mf.optim, CLASS[kind])(params, **HYPER[kind])
    assert _step_and_compare(mf, kind, opt, params, calls) == _singles(kind, params)


@pytest.mark.parametrize("kind", KINDS)
def test_three_tables_are_three_single_calls(mf, calls, monkeypatch, kind):
    monkeypatch.delenv("MF_UPDATE_PAIR", raising=False)
    params = _tables([32, 32, 32], seed=5)
    opt = getattr(mf.optim, CLASS[kind])(params, **HYPER[kind])
    assert _step_and_compare(mf, kind, opt, params, calls) == _singles(kind, params)


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_pending_is_no_call(mf, calls, monkeypatch, kind):
    monkeypatch.delenv("MF_UPDATE_PAIR", raising=False)
    params = _tables([32, 32], seed=6)
    opt = getattr(mf.optim, CLASS[kind])(params, **HYPER[kind])
    for p in params:
        p._mf_pending.clear()
    assert _step_and_compare(mf, kind, opt, params, calls) == []
    if kind == "adam":
        assert [opt.state[p]["step"] for p in params] == [0, 0]                  # the step does not move
