"""Cases of the dense (unmined) loss at which a workgroup of the three sweeps streams SEVERAL tiles, shared by
tests/test_dense_sweep_cpu.py (the cases themselves, checked without a GPU) and tests/test_gpu_dense_sweeps.py.

csrc/mf_loss_dense.hip splits the streamed axis of the forward, dU and dV sweeps into ranges of ``tps`` tiles per workgroup
(split_geometry, csrc/mf_loss_cols.h, applied in csrc/mf_loss_ws.h; a tile is 32 columns).  With four waves per workgroup ``tps`` > 1 needs Bp * Np > 2^21, above every other
dense case that is compared with a reference.  What a workgroup does depends on its tile count: one tile skips the
pipelined loop, two take the first iteration and the tail, three or more enter the loop unrolled by two tiles, five wrap
the forward's 4-deep side-input ring, four wrap the 3-slot ring of the d = 32 backward, and the last split may be shorter
than the others.  ``SHAPES`` names one shape per such path; ``plan`` reads the geometry the library would launch
(mf_loss_plan), so that a retuned split_geometry fails the tests instead of quietly returning them to one tile.

Two input families, seeded:

* ``random_case``: unit rows, per-column logQ, (sigma, margin) = (3.0, 0.25) -- the loss VALUE of all seven kinds and the
  gradients of the four smooth ones.
* ``lattice_case``: rows with entries in {-2 .. 2} * 2^-s, no logQ, sigma = 2.  Every logit is then a multiple of the step
  sigma * 2^-(2s+1) and exact in fp32, the margins sit half a step off that lattice, and so no hinge argument comes closer
  to its kink than half a step: a hinge gradient (a step function of the logit) can be compared on ALL rows.  With random
  inputs at these sizes hundreds of rows hold an element within rounding of its kink.

The reference is oracle.losses.loss in float64, its logits and masks evaluated once per case (``reference``).
"""
from __future__ import annotations

import contextlib
import ctypes
import functools

import numpy as np
import torch

from oracle import losses as ol
from tests import _golden_util as gu

WIDTHS = (32, 64, 128, 256)
# (B, N): ragged on purpose (B no multiple of 128, N no multiple of 32) -> ((tps, tiles in the last split) of the
# forward and dU, the same of dV), what it reaches
SHAPES = {
    (1020, 4090): ((2, 2), (2, 2), "first iteration + tail only"),
    (1990, 3050): ((3, 3), (3, 1), "one loop trip, single-tile tail; dV: last split of one tile"),
    (1500, 4400): ((4, 4), (4, 4), "one loop trip, two-tile tail; the 3-slot ring of d = 32 wraps"),
    (2990, 2990): ((5, 1), (5, 1), "the side-input ring wraps; last split of ONE tile; N == B"),
    (2000, 5190): ((6, 2), (5, 4), "two loop trips; last split of two tiles"),
    (900, 12000): ((6, 4), (6, 2), "few user blocks, long item axis"),
    # Both axes are padded to 128, so the last ONE TO THREE tiles of a sweep may hold padding only -- in every short last
    # split above they do, and a sweep that dropped its last tile there would lose nothing.  Here tile 95, alone in
    # the last split of all three sweeps, holds the real rows / columns 3040 .. 3059.
    (3060, 3060): ((5, 1), (5, 1), "as 2990 x 2990, with real rows and columns in the one-tile last split"),
}
RING_SHAPE = (2990, 2990)          # tps = 5, one-tile last split: the fused-forward and repeatability tests
OLD_SHAPES = ((256, 512), (200, 400), (1024, 2048), (768, 1536), (700, 1600))     # the dense cases of the older tests

SMOOTH = ("AlignmentLoss", "InfomationNoiseContrastiveEstimationLoss", "MutualInformationNeuralEstimationLoss",
          "PairwiseLogisticLoss")
HINGE = ("ContrastiveLoss", "AlignmentContrastiveLoss", "PairwiseHingeLoss")
P = 4
XB = 128                           # rows of the kept axis per workgroup (4 waves x 32)


def plan(lib, b, n, d, num_negatives=0):
    """mf_loss_plan as a dict; ``last_*``: tiles in the last split."""
    out = (ctypes.c_int64 * 8)()
    rc = lib.mf_loss_plan(b, n, d, num_negatives, out)
    assert rc == 0, (rc, lib.mf_last_error())
    names = ("mined", "nsplit_f", "tps_f", "nsplit_u", "tps_u", "nsplit_v", "tps_v")
    p = dict(zip(names, list(out)[:7]))
    p.update(last_f=out[7] & 0xFFFFF, last_u=(out[7] >> 20) & 0xFFFFF, last_v=out[7] >> 40)
    return p


def assert_plan(lib, b, n, d):
    """the geometry ``SHAPES`` promises for this case"""
    p = plan(lib, b, n, d)
    (tps_f, last_f), (tps_v, last_v), what = SHAPES[(b, n)]
    got = (p["mined"], p["tps_f"], p["last_f"], p["tps_u"], p["last_u"], p["tps_v"], p["last_v"])
    assert got == (0, tps_f, last_f, tps_f, last_f, tps_v, last_v), ((b, n, d), what, p)
    return p


def _ids_and_targets(b, n, g):
    t = {
        "target": torch.randint(-2, 6, (b,), generator=g),
        "item_idx": torch.randint(1, n // 2 + 1, (n,), generator=g),         # N / 2 values: duplicates, accidental hits
        "pos_idx": torch.randint(0, n // 2 + 1, (b, P), generator=g),
    }
    t["pos_idx"][:, 0] = t["item_idx"][:b]
    return t


@functools.lru_cache(maxsize=2)
def random_case(b, n, d):
    g = torch.Generator().manual_seed(1000 * d + b + n)
    t = {"u": torch.nn.functional.normalize(torch.randn(b, d, generator=g), dim=-1),
         "v": torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)}
    t.update(_ids_and_targets(b, n, g))
    t["logq"] = torch.log(torch.rand(n, generator=g) * 0.9 + 0.05)
    t["sigma"] = 3.0
    t["margin"] = dict.fromkeys(ol.KINDS, 0.25)
    return t


def lattice_shift(d):
    return 3 if d <= 64 else 4


@functools.lru_cache(maxsize=2)
def lattice_case(b, n, d):
    g = torch.Generator().manual_seed(2000 * d + b + n)
    s = lattice_shift(d)
    t = {"u": torch.randint(-2, 3, (b, d), generator=g).float() * 2.0 ** -s,
         "v": torch.randint(-2, 3, (n, d), generator=g).float() * 2.0 ** -s}
    t.update(_ids_and_targets(b, n, g))
    t["logq"] = None
    t["sigma"] = sigma = 2.0
    t["step"] = step = sigma * 2.0 ** -(2 * s + 1)
    lg = ol.logits_fn(t["u"].double(), t["v"].double(), t["target"].double(), sigma)
    med = float(lg[t["target"] != 0].abs().median())
    contrastive = round(med / step) * step + 0.5 * step
    t["margin"] = dict.fromkeys(ol.KINDS, contrastive)
    t["margin"].update(PairwiseHingeLoss=0.5 * step, PairwiseLogisticLoss=0.5 * step)
    return t


def hinge_arguments(t, lg, kind):
    """the relu's argument of a hinge kind, [B, N], from logits ``lg``"""
    m = t["margin"][kind]
    if kind == "PairwiseHingeLoss":
        return lg - lg.diagonal()[:, None] + m
    return lg + torch.sign(t["target"]).to(lg.dtype)[:, None] * m


@contextlib.contextmanager
def _shared_logits_and_masks():
    """oracle.losses.loss with its two shared intermediates evaluated once: the kinds of one case see the same logits
    (one autograd graph: differentiate with retain_graph) and the same hit masks."""
    logits_fn, negative_masks = ol.logits_fn, ol.negative_masks
    ol.logits_fn, ol.negative_masks = functools.lru_cache(maxsize=1)(logits_fn), functools.lru_cache(maxsize=1)(negative_masks)
    try:
        yield
    finally:
        ol.logits_fn, ol.negative_masks = logits_fn, negative_masks


def reference(t, kinds, grad_kinds, dtype=torch.float64, shared=True):
    """{kind: (value, du, dv)} of oracle.losses.loss at ``dtype`` (du = dv = None outside ``grad_kinds``)."""
    u, v = t["u"].to(dtype).requires_grad_(), t["v"].to(dtype).requires_grad_()
    tf = t["target"].to(dtype)
    logq = None if t["logq"] is None else t["logq"].to(dtype)
    out = {}
    with _shared_logits_and_masks() if shared else contextlib.nullcontext():
        for kind in kinds:
            val = ol.loss(kind, u, v, tf, item_idx=t["item_idx"], pos_idx=t["pos_idx"], sigma=t["sigma"],
                          margin=t["margin"][kind], logq=logq)
            du = dv = None
            if kind in grad_kinds:
                du, dv = (x.numpy() for x in torch.autograd.grad(val, (u, v), retain_graph=shared))
            out[kind] = (float(val.detach()), du, dv)
    return out


# ------------------------------------------------------------------------------ the checks ---
def value_bar(want, sigma, target):
    """the project's loss tolerance AND the north-star bar, whichever is tighter"""
    return min(gu.loss_tolerance(want, sigma, target), 1e-4 * sigma * max(1.0, abs(want)))


def assert_value_close(got, want, sigma, target, what):
    if not np.isfinite(want):
        assert got == want or (np.isnan(got) and np.isnan(want)), (what, got, want)
        return
    assert abs(got - want) <= value_bar(want, sigma, target), (what, got, want, abs(got - want), value_bar(want, sigma, target))


def where_streamed(index, tps):
    """(split, tile within the split) of the sweep that STREAMS the axis this row lies on"""
    tile = int(index) // 32
    return tile // tps, tile % tps


def grad_excess(got, want, sigma, base=1e-4, per_sigma=5e-6, floor=1e-5):
    """per row, the largest error in units of what _golden_util.assert_grads_close allows (its defaults)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max(axis=1, keepdims=True)
    allowed = (base + per_sigma * sigma) * (np.abs(want) + scale) + floor * sigma
    return (np.abs(got - want) / allowed).max(axis=1)


def assert_grads_close_located(got, want, sigma, what, side, p, floor_scale=1.0):
    """_golden_util.assert_grads_close over ALL rows; a failure names the worst row and where the sweeps hold it.
    ``side``: "du" (a user row: kept by the forward / dU workgroup i // 128, streamed by dV) or "dv" (an item row: kept by
    the dV workgroup j // 128, streamed by the forward and dU).  ``floor_scale``: the absolute floor of the bar times this --
    |g| where ``want`` is g x the gradient (a backward under a non-unit grad_out); the relative part scales by itself."""
    floor = 1e-5 * floor_scale
    try:
        gu.assert_grads_close(got, want, sigma, what, floor=floor)
    except AssertionError as e:
        ex = grad_excess(got, want, sigma, floor=floor)
        bad = np.nonzero(ex > 1.0)[0]
        r = int(np.argmax(ex))
        if side == "du":
            s, k = where_streamed(r, p["tps_v"])
            held = f"user block {r // XB} of the forward/dU grid; in dV: split {s} of {p['nsplit_v']}, tile {k} of {p['tps_v']}"
            splits = sorted({where_streamed(i, p["tps_v"]) for i in bad})
        else:
            s, k = where_streamed(r, p["tps_u"])
            held = (f"item block {r // XB} of the dV grid; in the forward/dU: split {s} of {p['nsplit_u']}, "
                    f"tile {k} of {p['tps_u']}")
            splits = sorted({where_streamed(i, p["tps_u"]) for i in bad})
        tiles_in_split = sorted({k for _, k in splits})
        msg = (f"{what}: {len(bad)} rows of {side} off; worst row {r} ({ex[r]:.3g} x the allowed error) -- {held}; "
               f"first bad rows {bad[:8].tolist()}, tiles-within-split of all bad rows {tiles_in_split[:16]}, "
               f"(split, tile) of the first {splits[:8]}")
        raise AssertionError(msg) from e
