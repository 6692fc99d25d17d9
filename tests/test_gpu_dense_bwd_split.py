"""GPU: the split backward sweeps of the dense loss at d = 128 (csrc/mf_bf_split.h, loss_bwd_dense_kernel's SPLIT variants)
against oracle.losses.loss in float64, against the fp32 sweeps, and against themselves.

dU and dV contract on the bf16 matrix cores: both operands in three bf16 pieces, the six leading piece products accumulated
in fp32.  Mode 2 (serve wherever d = 128) is forced and restored by a fixture, and every case asserts bit 1 of
``mf_loss_bwd_path`` on the workspace its backward used: a silent return to the fp32 sweeps fails the test.  Shapes, input
families and bars are those of tests/_dense_cases.py; the runs served by the distinct-column plan take their ids from
tests/test_gpu_dense_dedup.py (real copies, one column of weight ~700: a weighted G' is split)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests import _dense_cases as dc
from tests import test_gpu_dense_dedup as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
INFONCE = "InfomationNoiseContrastiveEstimationLoss"
LOGISTIC = "PairwiseLogisticLoss"
# tiles a workgroup of the sweeps streams (tests/_dense_cases.py): one; two; three, dV's last split of one; five, N = B; real
# rows in the one-tile last split
SHAPES = ((256, 512), (1020, 4090), (1990, 3050), (2990, 2990), (3060, 3060))
PATH_COLS, PATH_SPLIT = 1, 2


@pytest.fixture(autouse=True)
def _few_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


@pytest.fixture()
def split_always(mf):
    lib = mf._lib.lib()
    lib.mf_set_dense_bwd_split(2)
    yield lib
    lib.mf_set_dense_bwd_split(1)
    lib.mf_set_dense_dedup(1)


def _to_dev(t):
    return {k: x.to(DEV) for k, x in t.items() if isinstance(x, torch.Tensor)}


def _run_gpu(mf, kind, t, dev, retain=False):
    """(loss, du, dv, path of the backward, [the graph's (value, u, v) when retained])"""
    u, v = dev["u"].clone().requires_grad_(), dev["v"].clone().requires_grad_()
    fn = getattr(mf.losses, kind)(num_negatives=0, sigma=t["sigma"], margin=t["margin"][kind])
    val = fn(u, v, dev["target"], item_idx=dev["item_idx"], pos_idx=dev["pos_idx"], logq=dev.get("logq"))
    ws = val.grad_fn.saved_tensors[2]                     # the workspace of this forward (kept by the autograd node)
    val.backward(retain_graph=retain)
    path = mf._lib.lib().mf_loss_bwd_path(ws.data_ptr())
    return (val.detach(), u.grad.clone(), v.grad.clone(), path) + ((val, u, v),) * retain


def _served_ids(b, n):
    return "heavy" if n >= 1024 else "half"               # (heavy marks 700 columns: it needs more than that)


@functools.lru_cache(maxsize=2)
def _served_case(family, b, n):
    return dd.build_case(family, _served_ids(b, n), b, n, seed=11 + b + n)


# ------------------------------------------------------------------------ 1. the float64 oracle ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_sweeps_match_float64_oracle(mf, split_always, shape, plan):
    b, n = shape
    lib = split_always
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    p = dc.plan(lib, b, n, D)
    for family, kinds, grad_kinds in (("random", ol.KINDS, dc.SMOOTH), ("lattice", dc.HINGE, dc.HINGE)):
        if served:
            t = _served_case(family, b, n)
        else:
            t = dc.random_case(b, n, D) if family == "random" else dc.lattice_case(b, n, D)
        dev = _to_dev(t)
        got = {kind: _run_gpu(mf, kind, t, dev) for kind in kinds}
        want = dc.reference(t, kinds, grad_kinds)
        for kind in kinds:
            what = f"split {plan} {family} {kind} B={b} N={n}"
            val, du, dv, path = got[kind]
            if kind != "AlignmentLoss":                   # (no sweep runs for it)
                assert path & PATH_SPLIT, (what, path)
                assert bool(path & PATH_COLS) == served, (what, path)
            dc.assert_value_close(float(val.cpu()), want[kind][0], t["sigma"], t["target"].numpy(), what)
            if kind in grad_kinds:
                dc.assert_grads_close_located(du.cpu().numpy(), want[kind][1], t["sigma"], what, "du", p)
                dc.assert_grads_close_located(dv.cpu().numpy(), want[kind][2], t["sigma"], what, "dv", p)


# ---------------------------------------------------------------------- 2. no worse than fp32 ---
def test_split_gradients_are_no_worse_than_the_fp32_sweeps(mf, split_always):
    """E = the worst error against float64 in units of the gradient bar (_dense_cases.grad_excess).  A CPU emulation of the
    scheme (bf16 casts, B = 2048, N = 4096) gives E(six products) = 0.3 x E(fp32 matmul), and at least 4 x with any one
    second-order product dropped: the margin of 2 separates the two."""
    lib = split_always
    b, n = 1020, 4090
    t = dc.random_case(b, n, D)
    dev = _to_dev(t)
    kinds = (INFONCE, LOGISTIC)
    want = dc.reference(t, kinds, kinds)
    for kind in kinds:
        err = {}
        for mode in (0, 2):
            lib.mf_set_dense_bwd_split(mode)
            _, du, dv, path = _run_gpu(mf, kind, t, dev)
            assert bool(path & PATH_SPLIT) == (mode == 2), (kind, mode, path)
            err[mode] = tuple(float(dc.grad_excess(g.cpu().numpy(), w, t["sigma"]).max()) for g, w in ((du, want[kind][1]), (dv, want[kind][2])))
        for side, e_fp32, e_split in zip(("du", "dv"), err[0], err[2]):
            print(f"{kind} {side}: E(fp32) = {e_fp32:.4g}, E(split) = {e_split:.4g}")
            assert e_fp32 > 0 and e_split <= 2 * e_fp32, (kind, side, f"E(split) = {e_split:.6g}", f"E(fp32) = {e_fp32:.6g}")


# ---------------------------------------------------------------------------- 3. repeatability ---
@pytest.mark.parametrize("plan", ["plan-off", "plan-served"])
def test_split_sweeps_are_repeatable(mf, split_always, plan):
    """a second forward + backward, and a second backward on a retained graph, give the same bits"""
    lib = split_always
    b, n = dc.RING_SHAPE
    served = plan == "plan-served"
    lib.mf_set_dense_dedup(2 if served else 0)
    for kind, family in ((INFONCE, "random"), ("PairwiseHingeLoss", "lattice")):
        if served:
            t = _served_case(family, b, n)
        else:
            t = dc.random_case(b, n, D) if family == "random" else dc.lattice_case(b, n, D)
        dev = _to_dev(t)
        first = _run_gpu(mf, kind, t, dev)
        again = _run_gpu(mf, kind, t, dev, retain=True)
        assert first[3] & PATH_SPLIT and again[3] & PATH_SPLIT and bool(first[3] & PATH_COLS) == served, (first[3], again[3])
        for x, y, what in zip(first[:3], again[:3], ("loss", "du", "dv")):
            assert torch.equal(x, y), (kind, plan, what, "second forward + backward")
        val, u, v = again[4]
        u.grad = v.grad = None
        val.backward()
        assert torch.equal(u.grad, first[1]) and torch.equal(v.grad, first[2]), (kind, plan, "second backward on a retained graph")


def test_fp32_sweeps_are_intact_after_the_split_ones(mf, split_always):
    """mode 0 after mode 2 gives the bits of a mode-0 run before it"""
    lib = split_always
    b, n = 1020, 4090
    t = dc.random_case(b, n, D)
    dev = _to_dev(t)
    runs = []
    for mode in (0, 2, 0):
        lib.mf_set_dense_bwd_split(mode)
        runs.append(_run_gpu(mf, INFONCE, t, dev))
    assert [bool(r[3] & PATH_SPLIT) for r in runs] == [False, True, False], [r[3] for r in runs]
    for x, y, what in zip(runs[0][:3], runs[2][:3], ("loss", "du", "dv")):
        assert torch.equal(x, y), what
    assert torch.equal(runs[0][0], runs[1][0])            # the forward is the same code on every path
