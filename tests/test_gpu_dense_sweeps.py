"""GPU: the dense (unmined) loss where a workgroup of the forward, dU and dV sweeps streams SEVERAL tiles
(tests/_dense_cases.py names the paths), against oracle.losses.loss in float64 on the CPU.

Every other dense comparison of the suite gives each workgroup one tile (Bp * Np <= 2^21), except the full-size
training step (InfoNCE, d = 128, tps = 64).  Here: tile counts 2 .. 6, short last splits, all seven kinds, all four
widths -- the pipelined forward loop, the 3-slot ring of the d = 32 backward, the recomputing dV of d = 64 with its
coefficient prefetch, the G' stash of d = 128 / 256.  No row is left out of any comparison and no tolerance comes from
the kernels: the hinge kinds run on a lattice where their kinks are half a step away (tests/test_dense_sweep_cpu.py)."""
from __future__ import annotations

import pytest
import torch

from oracle import losses as ol
from tests import _dense_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(b, n, d) for (b, n) in dc.SHAPES for d in dc.WIDTHS]
ids = lambda c: "x".join(map(str, c))  # noqa: E731


@pytest.fixture(autouse=True)
def _few_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


def _to_dev(t):
    return {k: x.to(DEV) for k, x in t.items() if isinstance(x, torch.Tensor)}


def _loss_fn(mf, kind, t):
    return getattr(mf.losses, kind)(num_negatives=0, sigma=t["sigma"], margin=t["margin"][kind])


def _run_gpu(mf, kind, t, dev):
    u, v = dev["u"].clone().requires_grad_(), dev["v"].clone().requires_grad_()
    val = _loss_fn(mf, kind, t)(u, v, dev["target"], item_idx=dev["item_idx"], pos_idx=dev["pos_idx"], logq=dev.get("logq"))
    val.backward()
    return val.detach(), u.grad, v.grad


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_dense_sweeps_match_float64_oracle(mf, case):
    b, n, d = case
    p = dc.assert_plan(mf._lib.lib(), b, n, d)
    for family, kinds, grad_kinds in (("random", ol.KINDS, dc.SMOOTH), ("lattice", dc.HINGE, dc.HINGE)):
        t = (dc.random_case if family == "random" else dc.lattice_case)(b, n, d)
        dev = _to_dev(t)
        got = {kind: _run_gpu(mf, kind, t, dev) for kind in kinds}           # (queued before the CPU computes the reference)
        want = dc.reference(t, kinds, grad_kinds)
        for kind in kinds:
            what = f"{family} {kind} B={b} N={n} d={d} (tps {p['tps_f']}/{p['tps_u']}/{p['tps_v']}, " \
                   f"last {p['last_f']}/{p['last_u']}/{p['last_v']})"
            val, du, dv = got[kind]
            dc.assert_value_close(float(val.cpu()), want[kind][0], t["sigma"], t["target"].numpy(), what)
            if kind in grad_kinds:
                dc.assert_grads_close_located(du.cpu().numpy(), want[kind][1], t["sigma"], what, "du", p)
                dc.assert_grads_close_located(dv.cpu().numpy(), want[kind][2], t["sigma"], what, "dv", p)


@pytest.mark.parametrize("d", dc.WIDTHS)
def test_fused_forward_equals_single_kinds_with_a_wrapping_ring(mf, d):
    """The all-kinds forward is another instantiation of the sweep (every statistic at once, another interleave): at
    tps = 5 with a one-tile last split it gives the seven single-kind values, bit for bit."""
    b, n = dc.RING_SHAPE
    p = dc.assert_plan(mf._lib.lib(), b, n, d)
    assert (p["tps_f"], p["last_f"]) == (5, 1)
    t = dc.random_case(b, n, d)
    dev = _to_dev(t)
    args = dict(item_idx=dev["item_idx"], pos_idx=dev["pos_idx"], logq=dev["logq"])
    fused = mf.losses.fused_losses(dev["u"], dev["v"], dev["target"], num_negatives=0, sigma=t["sigma"], margin=0.25, **args)
    for kind in ol.KINDS:
        single = _loss_fn(mf, kind, t)(dev["u"], dev["v"], dev["target"], **args)
        assert float(fused[kind]) == float(single), (kind, d, float(fused[kind]), float(single))


@pytest.mark.parametrize("d", dc.WIDTHS)
def test_dense_sweeps_are_repeatable(mf, d):
    """No atomics on the dense path: a second forward + backward gives the same bits, and so does a second backward on a
    retained graph (the logit stash survives dU writing the G' stash)."""
    b, n = dc.RING_SHAPE
    dc.assert_plan(mf._lib.lib(), b, n, d)
    for kind, t in (("InfomationNoiseContrastiveEstimationLoss", dc.random_case(b, n, d)),
                    ("PairwiseHingeLoss", dc.lattice_case(b, n, d))):
        dev = _to_dev(t)
        first = _run_gpu(mf, kind, t, dev)
        again = _run_gpu(mf, kind, t, dev)
        for x, y, name in zip(first, again, ("loss", "du", "dv")):
            assert torch.equal(x, y), (kind, d, name, "second forward + backward")
        u, v = dev["u"].clone().requires_grad_(), dev["v"].clone().requires_grad_()
        val = _loss_fn(mf, kind, t)(u, v, dev["target"], item_idx=dev["item_idx"], pos_idx=dev["pos_idx"], logq=dev.get("logq"))
        val.backward(retain_graph=True)
        du1, dv1 = u.grad.clone(), v.grad.clone()
        u.grad = v.grad = None
        val.backward()
        assert torch.equal(val.detach(), first[0]) and torch.equal(du1, first[1]) and torch.equal(dv1, first[2]), (kind, d)
        assert torch.equal(u.grad, du1) and torch.equal(v.grad, dv1), (kind, d, "second backward on a retained graph")
