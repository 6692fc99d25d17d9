"""CPU: the cases of tests/_dense_cases.py are what the GPU tests take them for -- the split geometry they name, a lattice
on which no hinge element is near its kink, and bars a correct fp32 evaluation of the same formulas stays inside."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import chain, losses as ol
from tests import _dense_cases as dc
from tests import _golden_util as gu

CASES = [(b, n, d) for (b, n) in dc.SHAPES for d in dc.WIDTHS]
ids = lambda c: "x".join(map(str, c))  # noqa: E731


@pytest.fixture(autouse=True)
def _few_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


def test_every_case_reaches_the_path_it_is_named_for(mf):
    lib = mf._lib.lib()
    for b, n, d in CASES:
        p = dc.assert_plan(lib, b, n, d)
        assert b % dc.XB and n % dc.XB, (b, n)                                 # both axes end inside a workgroup's block
        assert n % 32 or (b, n) == (900, 12000), (b, n)                        # ... and, but for one, inside a tile
        assert (p["nsplit_f"] - 1) * p["tps_f"] + p["last_f"] == -(-n // dc.XB) * dc.XB // 32
        assert (p["nsplit_v"] - 1) * p["tps_v"] + p["last_v"] == -(-b // dc.XB) * dc.XB // 32
    reached = {(t, last) for (f, v, _) in dc.SHAPES.values() for (t, last) in (f, v)}
    assert {t for t, _ in reached} == {2, 3, 4, 5, 6} and {(3, 1), (5, 1), (6, 2)} <= reached
    # a short last split whose LAST tile is not padding alone, on the item axis (forward, dU) and on the user axis (dV)
    assert any(f[1] < f[0] and n % dc.XB > dc.XB - 32 for (b, n), (f, v, _) in dc.SHAPES.items())
    assert any(v[1] < v[0] and b % dc.XB > dc.XB - 32 for (b, n), (f, v, _) in dc.SHAPES.items())
    assert any(b == n for b, n in dc.SHAPES) and dc.RING_SHAPE in dc.SHAPES and dc.SHAPES[dc.RING_SHAPE][0] == (5, 1)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_lattice_logits_are_exact_and_no_hinge_element_is_near_its_kink(case):
    b, n, d = case
    t = dc.lattice_case(b, n, d)
    step = t["step"]
    lg64 = ol.logits_fn(t["u"].double(), t["v"].double(), t["target"].double(), t["sigma"])
    # exact in fp32: every partial sum is an integer multiple of 2^-2s below 2^24 of them, in ANY order -- torch's on the
    # whole matrix, and the kernel's own (the fmaf chain, a serial C loop) on every 16th user against all items
    lg32 = ol.logits_fn(t["u"], t["v"], t["target"].float(), t["sigma"])
    assert torch.equal(lg32.double(), lg64)
    rows = np.arange(0, b, 16)
    lgc = chain.logits(t["u"].numpy()[rows], t["v"].numpy(), t["target"].numpy()[rows], t["sigma"], None)
    assert np.array_equal(lgc.astype(np.float64), lg64.numpy()[rows])
    assert float((lg64 / step - (lg64 / step).round()).abs().max()) == 0.0      # every logit on the lattice
    valid = ol.negative_masks(t["item_idx"], t["pos_idx"], b) & (t["target"] != 0)[:, None]
    assert int(valid.sum()) > 0.9 * int((t["target"] != 0).sum()) * n
    for kind in ("ContrastiveLoss", "PairwiseHingeLoss"):
        x = dc.hinge_arguments(t, lg64, kind)[valid]
        assert float(x.abs().min()) >= 0.5 * step, (case, kind, float(x.abs().min()), step)
        active = float((x > 0).double().mean())
        assert 0.2 <= active <= 0.8, (case, kind, active)
    assert t["margin"]["AlignmentContrastiveLoss"] == t["margin"]["ContrastiveLoss"]


def test_shared_reference_is_the_oracle_loss():
    """``reference`` evaluates the logits and masks once for all kinds.  That changes no bit of any value; autograd may
    add the few contributions a leaf receives (norms, products, the alignment term) in another order: float64 rounding."""
    for t in (dc.random_case(300, 700, 64), dc.lattice_case(300, 700, 128)):
        a = dc.reference(t, ol.KINDS, ol.KINDS, shared=True)
        c = dc.reference(t, ol.KINDS, ol.KINDS, shared=False)
        for kind in ol.KINDS:
            assert a[kind][0] == c[kind][0], kind
            for x, y in zip(a[kind][1:], c[kind][1:]):
                assert np.abs(x - y).max() <= 2.0 ** -48 * np.abs(y).max(), kind


# the widest and the narrowest shape at every width, and each remaining shape at one width: every shape and every width
# is visited, inside the suite's time
FP32_CASES = [(b, n, d) for d in dc.WIDTHS for (b, n) in ((2000, 5190), (1020, 4090))] + \
             [(1990, 3050, 32), (1500, 4400, 64), (2990, 2990, 128), (900, 12000, 256)]


@pytest.mark.parametrize("case", FP32_CASES, ids=ids)
def test_bars_are_reachable_by_a_correct_fp32_evaluation(case):
    """torch's fp32 evaluation of oracle.losses.loss against its fp64 one, under the bars the GPU tests apply: the bars
    leave a correct fp32 implementation room (the kernel's summation order differs from torch's: it must stay within the
    bars, not within torch's own error)."""
    b, n, d = case
    for family, kinds, grad_kinds in (("random", ol.KINDS, dc.SMOOTH), ("lattice", dc.HINGE, dc.HINGE)):
        t = (dc.random_case if family == "random" else dc.lattice_case)(b, n, d)
        want = dc.reference(t, kinds, grad_kinds)
        got = dc.reference(t, kinds, grad_kinds, dtype=torch.float32)
        p = {"tps_u": 1, "tps_v": 1, "nsplit_u": 0, "nsplit_v": 0}             # (only names rows in a failure message)
        for kind in kinds:
            what = f"{family} {kind} {case} fp32 vs fp64"
            dc.assert_value_close(got[kind][0], want[kind][0], t["sigma"], t["target"].numpy(), what)
            if kind in grad_kinds:
                dc.assert_grads_close_located(got[kind][1], want[kind][1], t["sigma"], what, "du", p)
                dc.assert_grads_close_located(got[kind][2], want[kind][2], t["sigma"], what, "dv", p)
                # room to spare: a correct fp32 evaluation uses at most a quarter of the gradient bar
                assert dc.grad_excess(got[kind][1], want[kind][1], t["sigma"]).max() <= 0.25, what
                assert dc.grad_excess(got[kind][2], want[kind][2], t["sigma"]).max() <= 0.25, what


def test_a_failure_names_the_row_and_where_the_sweeps_hold_it():
    want = np.ones((400, 8))
    got = want.copy()
    got[330, 3] = 1.5                                   # tile 10: with tps = 4, split 2, tile 2 of it
    p = {"tps_u": 4, "tps_v": 3, "nsplit_u": 9, "nsplit_v": 5}
    with pytest.raises(AssertionError, match=r"worst row 330 .*item block 2 .*split 2 of 9, tile 2 of 4"):
        dc.assert_grads_close_located(got, want, 1.0, "x", "dv", p)
    with pytest.raises(AssertionError, match=r"worst row 330 .*user block 2 .*split 3 of 5, tile 1 of 3"):
        dc.assert_grads_close_located(got, want, 1.0, "x", "du", p)
    dc.assert_grads_close_located(want, want, 1.0, "x", "du", p)
    # the located report applies the same criterion as the project's own check
    assert dc.grad_excess(got, want, 1.0)[330] > 1.0 and (np.delete(dc.grad_excess(got, want, 1.0), 330) == 0).all()
    with pytest.raises(AssertionError):
        gu.assert_grads_close(got, want, 1.0, "x")
