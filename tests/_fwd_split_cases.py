"""Cases of the split dense-loss forward (csrc/mf_bf_split.h, loss_fwd_dense_kernel's SPLIT variant), shared by
tests/test_dense_fwd_split_cpu.py (checked without a GPU) and tests/test_gpu_dense_fwd_split.py.

* ``SHAPES``: (B, N) at d = 128 with the forward's geometry each is chosen for; ``assert_geometry`` reads it from mf_loss_plan
  and mf_loss_cols_plan, so a retuned split_geometry fails the tests instead of quietly moving them to another path.
* ``precision_case`` / ``emulate``: the inputs of the precision test and the CPU emulation of the split score tile on them --
  the source of the factor that test uses.
"""
from __future__ import annotations

import ctypes
import functools

import torch

from oracle import losses as ol
from tests import _dense_cases as dc

D = 128
PATH_COLS, PATH_SPLIT = 1, 2
INFONCE = "InfomationNoiseContrastiveEstimationLoss"
LOGISTIC = "PairwiseLogisticLoss"
FWD_SPLIT_MIN_BN = 2048 * 4096     # mode 1 of mf_set_dense_fwd_split serves from B x N scores upward (csrc/mf_loss_dense.hip)
GATE_SHAPES = ((2040, 4100), (2050, 4096))     # B x N just below and just at the gate (8,364,000 and 8,396,800 against 8,388,608)

# (B, N) -> ((forward splits, tiles per split, tiles in the last split), what it reaches)
SHAPES = {
    (24, 40): ((4, 1, 1), "one partial user tile; Np = 128: one real item tile of 32 and one of 8 columns, two of padding only"),
    (24, 1030): ((36, 1, 1), "one partial user tile; tile 32 holds 6 real columns, tiles 33..35 none"),
    (300, 1030): ((36, 1, 1), "three user blocks, one-tile splits: the pipelined loop is skipped"),
    (1020, 4090): ((64, 2, 2), "two tiles per split: first iteration + tail"),
    (2990, 2990): ((20, 5, 1), "five tiles per split: the loop runs, the side-input ring wraps; a one-tile last split"),
}
ROUTE_SHAPE = (300, 1030)
STREAM_SHAPE = (1020, 4090)
RING_SHAPE = (2990, 2990)
PADDED_WIDTHS = (100, 65)

# The precision test: ``emulation_ratios(precision_case())`` gave r6 (six products) and r5 (the best of five) below on the
# CPU; the factor is their geometric mean (tests/test_dense_fwd_split_cpu.py reruns the emulation)
PRECISION_SHAPE = STREAM_SHAPE
PRECISION_SIGMA = 24.0
R6, R5 = 1.00, 3.05
FACTOR = 1.75


def plan_f(lib, b, n, d=D):
    p = dc.plan(lib, b, n, d)
    return p["nsplit_f"], p["tps_f"], p["last_f"]


def assert_geometry(lib, b, n):
    want, what = SHAPES[(b, n)]
    assert plan_f(lib, b, n) == want, ((b, n), what, plan_f(lib, b, n))
    # with every column distinct the column plan derives the same forward geometry
    out = (ctypes.c_int64 * 16)()
    assert lib.mf_loss_cols_plan(b, n, D, n, out) == 0
    assert (out[0], out[2], out[3]) == (1, want[0], want[1]), ((b, n), list(out))
    return want


def default_serves(b, n, d, num_negatives):
    """what mode 1 of the forward's switch serves"""
    return d == 128 and not (0 < num_negatives < n) and b * n >= FWD_SPLIT_MIN_BN


@functools.lru_cache(maxsize=1)
def precision_case():
    """``random_case`` at PRECISION_SHAPE under a sharp softmax: with sigma this large a row's G' is carried by its few largest
    logits and follows their error directly"""
    t = dict(dc.random_case(*PRECISION_SHAPE, D))
    t["sigma"] = PRECISION_SIGMA
    return t


# ------------------------------------------------------------------------ the emulation ---
def bf16_pieces(x):
    """fp32 -> three bf16 pieces (as fp32), each rounding what the pieces before it left (mbf_split3)"""
    out, r = [], x
    for _ in range(3):
        p = r.to(torch.bfloat16).to(torch.float32)
        out.append(p)
        r = r - p
    return out


PRODUCTS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))     # (item piece, user piece), the smallest first, as the kernel adds them


def scores(u, v, dropped=None):
    """u v^T [B, N] from the piece products with i + j <= 2 (exact products, fp32 accumulation), without ``dropped``"""
    up, vp = bf16_pieces(u), bf16_pieces(v)
    acc = torch.zeros(u.shape[0], v.shape[0], dtype=torch.float32)
    for vi, ui in PRODUCTS:
        if (vi, ui) != dropped:
            acc = acc + up[ui] @ vp[vi].T
    return acc


def logits_of_scores(t, s32):
    """the kernel's logit map in fp32 on fp32 scores: L = -sigma s_i ((|u_i|^2 + |v_j|^2) / 2 - S_ij) - logq_j"""
    u, v = t["u"], t["v"]
    half = 0.5 * ((u * u).sum(1)[:, None] + (v * v).sum(1)[None, :])
    lg = -(half - s32) * (torch.sign(t["target"]).float() * t["sigma"])[:, None]
    return lg if t["logq"] is None else lg - t["logq"][None, :]


def _grads_at(t, kind, lg32):
    """the float64 gradients of oracle.losses.loss with its logits shifted to the fp32 values ``lg32`` (None: as they are)"""
    u, v = t["u"].double().requires_grad_(), t["v"].double().requires_grad_()
    tf = t["target"].double()
    logq = None if t["logq"] is None else t["logq"].double()
    exact = ol.logits_fn

    def shifted(*a, **k):
        lg = exact(*a, **k)
        return lg if lg32 is None else lg + (lg32.double() - lg.detach())
    ol.logits_fn = shifted
    try:
        val = ol.loss(kind, u, v, tf, item_idx=t["item_idx"], pos_idx=t["pos_idx"], sigma=t["sigma"], margin=t["margin"][kind],
                      logq=logq)
        du, dv = torch.autograd.grad(val, (u, v))
    finally:
        ol.logits_fn = exact
    return float(val.detach()), du.numpy(), dv.numpy()


def emulate(t, kind):
    """E (``grad_excess``, worst row) of the gradients the loss gives when its score tile is an fp32 matmul, the six piece
    products, and five of them with each second-order product dropped in turn; the logit map runs in fp32 on those scores and
    everything behind the logits in float64.  {side: {"fp32": E, "six": E, "five": {dropped: E}}}"""
    _, du64, dv64 = _grads_at(t, kind, None)

    def excess(s32):
        _, du, dv = _grads_at(t, kind, logits_of_scores(t, s32))
        return tuple(float(dc.grad_excess(g, w, t["sigma"]).max()) for g, w in ((du, du64), (dv, dv64)))
    e32, e6 = excess(t["u"] @ t["v"].T), excess(scores(t["u"], t["v"]))
    e5 = {d: excess(scores(t["u"], t["v"], dropped=d)) for d in ((2, 0), (1, 1), (0, 2))}
    return {side: {"fp32": e32[k], "six": e6[k], "five": {d: e[k] for d, e in e5.items()}} for k, side in enumerate(("du", "dv"))}


def emulation_ratios(t, kinds=(INFONCE,)):
    """(r6, r5): the largest E(six products) / E(fp32) and the smallest E(five products) / E(fp32) over kinds and sides"""
    r6, r5 = 0.0, float("inf")
    for kind in kinds:
        for side, e in emulate(t, kind).items():
            assert e["fp32"] > 0, (kind, side)
            r6 = max(r6, e["six"] / e["fp32"])
            r5 = min(r5, min(e["five"].values()) / e["fp32"])
    return r6, r5
