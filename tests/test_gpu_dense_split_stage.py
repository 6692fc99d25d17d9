"""GPU: the staging of the split dense sweeps at d = 128 (csrc/mf_loss_dense.hip: the SPLIT loops of loss_bwd_dense_kernel
issue a tile's memory instructions inside the previous tile's contraction, four to each of its steps, and slice the next
tile's G' beside them), against oracle.losses.loss in float64, against the fp32 sweeps and against themselves.

Forward and backward split mode 2 are forced and restored by a fixture; every case asserts ``mf_loss_fwd_path`` and
``mf_loss_bwd_path`` on the workspace it used.  Shapes come from mf_loss_plan / mf_loss_cols_plan (asserted: a retuned
geometry fails here), chosen for what the staging does at a split's edges:

* splits of exactly 1, 2 and 3 tiles -- the prologue and the last iterations, where "two tiles ahead" names no tile;
* five tiles per split with a one-tile last split;
* (24, 1030), (300, 1030), (1020, 4090) with the column plan off and served; served, N' is no multiple of 32 in every case
  (asserted), so the last streamed tile's weights straddle N';
* the "heavy" ids (one column of weight ~700) with the r6 / r5 factor of tests/_bwd_split_cases.py;
* grad_out = -0.5; a workspace filled with 0xFF; two runs; split against the fp32 sweeps.
Bars, input families and the reference are those of tests/_dense_cases.py."""
from __future__ import annotations

import ctypes
import functools
import math

import pytest
import torch

from oracle import losses as ol
from tests import _bwd_split_cases as sc
from tests import _dense_cases as dc
from tests import test_gpu_dense_bwd_split_routes as rt
from tests import test_gpu_dense_dedup as dd

pytestmark = pytest.mark.gpu
D = sc.D
COLS, SPLIT, RECOMP = sc.PATH_COLS, sc.PATH_SPLIT, sc.PATH_RECOMP
INFONCE, LOGISTIC, HINGE = sc.INFONCE, sc.LOGISTIC, sc.HINGE
# (B, N) -> plan off: (dU tiles per split, in its last split), (dV the same); plan served: N' of the "heavy" ids (seed
# 11 + B + N) and the tiles per split of dU and dV that mf_loss_cols_plan gives for it
SHAPES = {
    (24, 1030): ((1, 1), (1, 1), 328, (1, 1)),
    (300, 1030): ((1, 1), (1, 1), 276, (1, 1)),
    (1020, 4090): ((2, 2), (2, 2), 2973, (2, 2)),
    (1990, 3050): ((3, 3), (3, 1), 1590, (2, 2)),
    (2990, 2990): ((5, 1), (5, 1), 1146, (2, 2)),
}
EDGE_SHAPES = ((300, 1030), (1020, 4090), (1990, 3050))     # 1, 2 and 3 tiles per split: the other tests' shapes


@pytest.fixture(autouse=True)
def _few_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


@pytest.fixture()
def split_both(mf):
    """forward and backward split wherever they can serve; every switch at its default afterwards"""
    lib = mf._lib.lib()
    lib.mf_set_dense_fwd_split(2)
    lib.mf_set_dense_bwd_split(2)
    yield lib
    lib.mf_set_dense_fwd_split(1)
    lib.mf_set_dense_bwd_split(1)
    lib.mf_set_dense_dedup(1)


@functools.lru_cache(maxsize=2)
def _heavy(family, b, n):
    return dd.build_case(family, "heavy", b, n, seed=11 + b + n)


def _case(family, b, n, served):
    return _heavy(family, b, n) if served else rt._case(family, b, n)


@functools.lru_cache(maxsize=None)
def _reference(family, b, n, served):
    """float64, once per case: the values of the family's kinds and the gradients of its trained ones (never written to)"""
    kinds, grad_kinds = {"random": (ol.KINDS, dc.SMOOTH), "lattice": (dc.HINGE, dc.HINGE)}[family]
    return dc.reference(_case(family, b, n, served), kinds, grad_kinds)


def _run(mf, kind, t, dev, scale=None):
    """(loss, du, dv, backward path, forward path)"""
    val, u, v, ws = rt._forward(mf, kind, t, dev)
    fpath = mf._lib.lib().mf_loss_fwd_path(ws.data_ptr())
    return (val.detach().clone(),) + rt._backward(mf, val, u, v, ws, scale=scale) + (fpath,)


def _assert_paths(got, served, what):
    assert got[3] == SPLIT | RECOMP | (COLS if served else 0), (what, "backward path", got[3])
    assert got[4] == SPLIT | (COLS if served else 0), (what, "forward path", got[4])


def _assert_geometry(lib, b, n, served):
    (tps_u, last_u), (tps_v, last_v), ncols, (ctps_u, ctps_v) = SHAPES[(b, n)]
    p = dc.plan(lib, b, n, D)
    assert (p["tps_f"], p["tps_u"], p["last_u"], p["tps_v"], p["last_v"]) == (tps_u, tps_u, last_u, tps_v, last_v), p
    if served:
        kept, _ = sc.copy_weights(_heavy("random", b, n))
        assert len(kept) == ncols and ncols % 32 != 0, (len(kept), ncols)
        out = (ctypes.c_int64 * 16)()
        assert lib.mf_loss_cols_plan(b, n, D, ncols, out) == 0
        assert out[0] == 1 and (out[5], out[7]) == (ctps_u, ctps_v), list(out)
    return p


# ------------------------------------------------------------------------ 1. the float64 oracle ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_staged_split_sweeps_match_float64_oracle(mf, split_both, shape, plan):
    b, n = shape
    lib = split_both
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    p = _assert_geometry(lib, b, n, served)
    for family, kinds, grad_kinds in rt.FAMILIES:
        t = _case(family, b, n, served)
        dev = rt._to_dev(t)
        got = {kind: _run(mf, kind, t, dev) for kind in kinds}
        want = _reference(family, b, n, served)
        for kind in kinds:
            what = f"staged split {plan} {family} {kind} B={b} N={n}"
            if kind != "AlignmentLoss":                       # (no sweep runs for it)
                _assert_paths(got[kind], served, what)
            dc.assert_value_close(float(got[kind][0].cpu()), want[kind][0], t["sigma"], t["target"].numpy(), what)
            if kind in grad_kinds:
                rt._check_grads(got[kind], want[kind], t, what, p)


# ------------------------------------------------------------- 2. a weighted G' keeps six products ---
def test_heavy_weights_keep_the_six_piece_products(mf, split_both):
    """tests/test_gpu_dense_bwd_split_routes.py's precision check with the forward split as well: E(split) within the factor
    between r6 (six products) and r5 (any five) of E(fp32) -- a stage that lost or misplaced a weight, or a piece product,
    lands beyond it."""
    lib = split_both
    assert abs(sc.FACTOR - math.sqrt(sc.R6 * sc.R5)) <= 0.005 and sc.R5 >= 2 * sc.R6
    b, n = sc.PRECISION_SHAPE
    lib.mf_set_dense_dedup(2)
    err = rt._excess_by_mode(mf, lib, sc.heavy_case("random", b, n), (INFONCE, LOGISTIC), (0, 2))
    bad = []
    for kind, by_mode in err.items():
        for side, e_fp32, e_split in zip(("du", "dv"), by_mode[0], by_mode[2]):
            print(f"{kind} {side}: E(fp32) = {e_fp32:.4g}, E(split) = {e_split:.4g}")
            if not (e_fp32 > 0 and e_split <= sc.FACTOR * e_fp32):
                bad.append((kind, side, f"E(split) = {e_split:.6g}", f"E(fp32) = {e_fp32:.6g}"))
    assert not bad, bad


# ---------------------------------------------------------------------------------- 3. grad_out ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_negative_grad_out(mf, split_both, shape, plan):
    b, n = shape
    served = plan == "plan-served"
    split_both.mf_set_dense_dedup(2 if served else 0)
    p = dc.plan(split_both, b, n, D)
    for kind, family in ((INFONCE, "random"), (LOGISTIC, "random"), (HINGE, "lattice")):
        t = _case(family, b, n, served)
        got = _run(mf, kind, t, rt._to_dev(t), scale=-0.5)
        what = f"grad_out = -0.5 {plan} {family} {kind} B={b} N={n}"
        _assert_paths(got, served, what)
        rt._check_grads(got, _reference(family, b, n, served)[kind], t, what, p, scale=-0.5)


# ------------------------------------------------------------------- 4. against themselves ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
@pytest.mark.parametrize("shape", EDGE_SHAPES + ((2990, 2990),), ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_runs_give_the_same_bits(mf, split_both, shape, plan):
    b, n = shape
    served = plan == "plan-served"
    split_both.mf_set_dense_dedup(2 if served else 0)
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = _case(family, b, n, served)
        dev = rt._to_dev(t)
        first, again = _run(mf, kind, t, dev), _run(mf, kind, t, dev)
        _assert_paths(first, served, (kind, plan))
        _assert_paths(again, served, (kind, plan))
        rt._same_bits(first, again, (kind, plan, shape, "second forward + backward"))


@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
@pytest.mark.parametrize("shape", ((24, 1030), (1020, 4090)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_workspace_of_ones_bits_gives_the_bits_of_a_clean_one(mf, split_both, shape, plan):
    """forward + backward through the C ABI on a workspace filled with 0xFF against one filled with 0x00: the stage reads
    ahead of the tiles it uses -- the last tile's block again, image tiles that are never contracted"""
    lib = split_both
    b, n = shape
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    ws = torch.empty(lib.mf_loss_ws_bytes(b, n, D, dc.P, 0), dtype=torch.uint8, device=rt.DEV)
    for kind, family in ((INFONCE, "random"), (HINGE, "lattice")):
        t = _case(family, b, n, served)
        dev = rt._to_dev(t)
        runs = {}
        for fill in (0x00, 0xFF):
            ws.fill_(fill)
            runs[fill] = rt._abi_run(mf, kind, t, dev, ws, b, n)
            assert runs[fill][3] == SPLIT | RECOMP | (COLS if served else 0), (kind, plan, fill, runs[fill][3])
            assert lib.mf_loss_fwd_path(ws.data_ptr()) == SPLIT | (COLS if served else 0)
            assert torch.isfinite(runs[fill][1]).all() and torch.isfinite(runs[fill][2]).all(), (kind, plan, fill)
        rt._same_bits(runs[0xFF], runs[0x00], (kind, plan, shape, "workspace of 0xFF against a clean one"))


# ------------------------------------------------------------------- 5. against the fp32 sweeps ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
@pytest.mark.parametrize("shape", ((1020, 4090), (1990, 3050)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_and_fp32_sweeps_agree(mf, split_both, shape, plan):
    """The two backward schemes contract the same G' of the same stash: their gradients differ by rounding only, so each
    lies within the gradient bar of the other (the bar the float64 comparison uses, taken around the fp32 sweeps' result)."""
    lib = split_both
    b, n = shape
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    p = dc.plan(lib, b, n, D)
    for kind, family in ((INFONCE, "random"), (LOGISTIC, "random"), (HINGE, "lattice")):
        t = _case(family, b, n, served)
        dev = rt._to_dev(t)
        split = _run(mf, kind, t, dev)
        _assert_paths(split, served, (kind, plan))
        lib.mf_set_dense_bwd_split(0)
        fp32 = _run(mf, kind, t, dev)
        lib.mf_set_dense_bwd_split(2)
        assert not fp32[3] & SPLIT, fp32[3]
        assert torch.equal(split[0], fp32[0])                 # one forward
        for side, g, w in (("du", split[1], fp32[1]), ("dv", split[2], fp32[2])):
            e = float(dc.grad_excess(g.cpu().numpy(), w.cpu().numpy(), t["sigma"]).max())
            print(f"{plan} {kind} {shape} {side}: split against fp32, {e:.4g} x the bar")
        rt._check_grads(split, (None, fp32[1].cpu().numpy(), fp32[2].cpu().numpy()), t, f"split against fp32 {plan} {kind} {shape}", p)
