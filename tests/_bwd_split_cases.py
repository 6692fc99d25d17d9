"""Cases of the split dense-loss backward (csrc/mf_bf_split.h, loss_bwd_dense_kernel's SPLIT variants) on the routes its
first tests never took, shared by tests/test_bwd_split_routes_cpu.py (the cases themselves, checked without a GPU) and
tests/test_gpu_dense_bwd_split_routes.py.

* ``SERVED`` / ``UNSERVED``: shapes on either side of the default switch (mode 1 serves d = 128, unmined, N >= 8192), with the
  geometry each is chosen for.  ``assert_geometry`` reads it from mf_loss_plan: a retuned split_geometry fails the tests.
* ``ROUTE_SHAPE`` / ``SMALL_SHAPE``: the shapes of the route, switch and poison tests under mode 2.
* builders of the inputs of single routes: CSR positives with the zero padding kept, a logQ table looked up by item id.
* ``emulate``: the CPU emulation of the contraction (torch bf16 casts) on a case's own G', weighted by the copy counts of the
  distinct-column plan -- the source of the factor the precision test on the plan-served case uses.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import losses as ol
from tests import _dense_cases as dc
from tests import test_gpu_dense_dedup as dd

D = 128
PATH_COLS, PATH_SPLIT, PATH_RECOMP = 1, 2, 4
INFONCE = "InfomationNoiseContrastiveEstimationLoss"
LOGISTIC = "PairwiseLogisticLoss"
HINGE = "PairwiseHingeLoss"
SPLIT_MIN_N = 8192                 # mode 1 of mf_set_dense_bwd_split serves from here (csrc/mf_loss_dense.hip)
COLS_MIN_N = 4096                  # mode 1 of mf_set_dense_dedup

# (B, N) at d = 128, unmined: (dU splits, tiles per split), (dV splits, tiles per split), the images have room of their own
SERVED = {
    (24, 8192): ((256, 1), (4, 1), True, "one X block; dV: four one-tile splits over user tiles, three of them padding only"),
    (128, 8192): ((256, 1), (4, 1), True, "Bp = B exactly"),
    (300, 8200): ((130, 2), (6, 2), False, "two tiles per split; tile 256 holds 8 real columns, tiles 257..259 none"),
}
# (B, N, d, num_negatives) -> the path its backward must report under the default switches
UNSERVED = {
    (24, 8191, 128, 0): (PATH_COLS, "one column below the threshold (the column plan serves from 4096)"),
    (300, 8191, 128, 0): (PATH_COLS, "one column below the threshold"),
    (64, 8192, 64, 0): (0, "d = 64 is never split"),
    (64, 8192, 128, 4): (0, "mined: no dense sweep runs"),
}
ROUTE_SHAPE = (300, 1030)          # Bp = 384, NT = 36, one-tile splits, images inside the G' stash
SMALL_SHAPE = (24, 1030)           # Bp = 128: images in their own room, dV's splits over padding only
STREAM_SHAPE = (1020, 4090)        # a workgroup streams two tiles (tests/_dense_cases.py)
ROUTE_GEOMETRY = {ROUTE_SHAPE: ((36, 1), (12, 1), False), SMALL_SHAPE: ((36, 1), (4, 1), True),
                  STREAM_SHAPE: ((64, 2), (16, 2), False)}
PADDED_WIDTHS = (100, 65)          # padded to 128 by the package: the image holds zero features
GRAD_OUTS = (2.5, -0.5, 2.0 ** -20)
COMBINATION = ((INFONCE, 0.75), (LOGISTIC, -1.5))
# The precision test on the plan-served case: ``emulation_ratios(heavy_case("random", *PRECISION_SHAPE))`` gave r6 (six
# products) and r5 (the best of five) below; the factor is their geometric mean (tests/test_bwd_split_routes_cpu.py reruns it)
PRECISION_SHAPE = ROUTE_SHAPE
R6, R5 = 1.10, 3.52
FACTOR = 1.97


def padded(x, to=128):
    return -(-x // to) * to


def images_own_room(b, n):
    """loss_ws (csrc/mf_loss_ws.h): the two operand images -- 24 KiB per 32-row tile -- live in the G' stash unless they do not
    fit it: 6 (BT + NT) <= BT NT in units of 4 KiB"""
    bt, nt = padded(b) // 32, padded(n) // 32
    return 6 * (bt + nt) > bt * nt


def assert_geometry(lib, b, n, want_u, want_v, own_room, d=D):
    p = dc.plan(lib, b, n, d)
    got = (p["mined"], (p["nsplit_u"], p["tps_u"]), (p["nsplit_v"], p["tps_v"]))
    assert got == (0, want_u, want_v), ((b, n, d), p)
    assert images_own_room(b, n) == own_room, (b, n)
    # every tile of both axes is streamed by exactly one split
    assert (p["nsplit_u"] - 1) * p["tps_u"] + p["last_u"] == padded(n) // 32
    assert (p["nsplit_v"] - 1) * p["tps_v"] + p["last_v"] == padded(b) // 32
    images = (padded(b) + padded(n)) // 32 * 3 * 32 * 128 * 2
    stashes = 2 * padded(b) * padded(n) * 4
    size = lib.mf_loss_ws_bytes(b, n, d, 0, 0)
    assert size > stashes + (images if own_room else 0), ((b, n), size)
    return p


def default_serves(n, d, num_negatives):
    """what mode 1 of the split switch serves"""
    return d == 128 and not (0 < num_negatives < n) and n >= SPLIT_MIN_N


def csr_of_padded(pos_idx):
    """(user_ids, pos_off, pos_items): user i's list is row i of ``pos_idx`` as it is, zeros included -- a padded 0 is looked up
    like any id on both routes, so the hit masks are the same bits"""
    b, p = pos_idx.shape
    return torch.arange(b, dtype=torch.int64), torch.arange(b + 1, dtype=torch.int64) * p, pos_idx.reshape(-1).clone()


@functools.lru_cache(maxsize=2)
def table_case(b, n):
    """``random_case`` whose logQ comes from a table over the item ids: (the case with logq = table[item_idx], the table)"""
    t = dict(dc.random_case(b, n, D))
    g = torch.Generator().manual_seed(31 + b + n)
    table = torch.log(torch.rand(int(t["item_idx"].max()) + 1, generator=g) * 0.9 + 0.05)
    t["logq"] = table[t["item_idx"]].contiguous()
    return t, table


def heavy_case(family, b, n):
    """the plan-served inputs of tests/test_gpu_dense_bwd_split.py: real copies, one id on ~700 columns"""
    assert n >= 1024
    return dd.build_case(family, "heavy", b, n, seed=11 + b + n)


# ------------------------------------------------------------------------ the emulation ---
def _bf16_pieces(x):
    """fp32 -> three bf16 pieces (as fp32), each rounding what the pieces before it left (mbf_split3)"""
    out, r = [], x
    for _ in range(3):
        p = r.to(torch.bfloat16).to(torch.float32)
        out.append(p)
        r = r - p
    return out


def _contract(a, g, dropped=None):
    """g @ a from the piece products a_i g_j with i + j <= 2 (fp32 accumulation), without ``dropped``"""
    ap, gp = _bf16_pieces(a), _bf16_pieces(g)
    acc = torch.zeros(g.shape[0], a.shape[1], dtype=torch.float32)
    for ai, gi in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)):           # the smallest first, as the kernel adds them
        if (ai, gi) != dropped:
            acc = acc + gp[gi] @ ap[ai]
    return acc


def copy_weights(t):
    """(kept columns, weight of each): column j is a copy iff its id's first column holds the same row and logQ bits"""
    ids = t["item_idx"].numpy()
    v = t["v"].numpy().view(np.int32)
    lq = (np.zeros(len(ids), np.float32) if t["logq"] is None else t["logq"].numpy()).view(np.int32)
    _, first_of, inv = np.unique(ids, return_index=True, return_inverse=True)
    f = first_of[inv]
    copy = (f != np.arange(len(ids))) & (v == v[f]).all(axis=1) & (lq == lq[f])
    rep = np.where(copy, f, np.arange(len(ids)))
    kept = np.nonzero(~copy)[0]
    weight = np.bincount(rep, minlength=len(ids))[kept]
    return torch.from_numpy(kept), torch.from_numpy(weight.astype(np.float32))


def _g_prime(t, kind, dtype):
    """dloss / dL [B, N] of oracle.losses.loss evaluated at ``dtype``, and the loss's gradients"""
    u, v = t["u"].clone().to(dtype).requires_grad_(), t["v"].clone().to(dtype).requires_grad_()     # (never the case's own)
    tf = t["target"].to(dtype)
    logq = None if t["logq"] is None else t["logq"].to(dtype)
    with dc._shared_logits_and_masks():
        lg = ol.logits_fn(u, v, tf, t["sigma"], logq)                         # the tensor the loss below differentiates through
        val = ol.loss(kind, u, v, tf, item_idx=t["item_idx"], pos_idx=t["pos_idx"], sigma=t["sigma"], margin=t["margin"][kind],
                      logq=logq)
        g, du, dv = torch.autograd.grad(val, (lg, u, v))
    return g.detach(), du.detach(), dv.detach()


def emulate(t, kind):
    """E (``grad_excess``, worst row) of the gradients an fp32 evaluation of G' gives when its two contractions -- dU: (G' x the
    copy counts) . v' over the distinct columns, dV: G'^T . u -- run as an fp32 matmul, as the six piece products, and as five
    of them with each second-order product dropped in turn.  Everything but the contraction is float64, so E is the error of
    G' in fp32 (common to all schemes) and of the contraction.  {side: {"fp32": E, "six": E, "five": {dropped: E}}}"""
    g64, du64, dv64 = _g_prime(t, kind, torch.float64)
    g32 = _g_prime(t, kind, torch.float32)[0]
    # dL_ij / du_i = sigma s_i (v_j - u_i), dL_ij / dv_j = sigma s_i (u_i - v_j): the kernels fold sigma s_i into G'
    coef = (t["sigma"] * torch.sign(t["target"]).double())[:, None]
    gk64, gk32 = g64 * coef, (g32.double() * coef).float()
    # A user's own column is no part of the plan-served contractions: its id masks every copy of it (G' = 0 there) and the
    # epilogue adds the diagonal term by itself (sum_parts_cols_kernel).  Without it, copies hold equal columns of G' -- same
    # row, same logQ, same mask, which goes by id -- and the distinct columns carry their copy counts.
    b = g64.shape[0]
    gk64[torch.arange(b), torch.arange(b)] = 0.0
    gk32[torch.arange(b), torch.arange(b)] = 0.0
    kept, weight = copy_weights(t)
    gw32 = gk32[:, kept] * weight[None, :]                                    # (rounded once more in fp32, as Gv *= Wv is)
    vk = t["v"][kept]
    exact_u = gk64 @ t["v"].double()
    assert float((exact_u - (gk64[:, kept] * weight.double()[None, :]) @ vk.double()).abs().max()) <= 1e-12 * float(exact_u.abs().max())
    exact_v = gk64.T @ t["u"].double()
    out = {}
    for side, a, g, exact, ref in (("du", vk, gw32, exact_u, du64), ("dv", t["u"], gk32.T.contiguous(), exact_v, dv64)):
        def excess(c):
            got = ref + (c.double() - exact)
            return float(dc.grad_excess(got.numpy(), ref.numpy(), t["sigma"]).max())
        out[side] = {"fp32": excess(g @ a), "six": excess(_contract(a, g)),
                     "five": {d: excess(_contract(a, g, dropped=d)) for d in ((2, 0), (1, 1), (0, 2))}}
    return out


def emulation_ratios(t, kinds=(INFONCE, LOGISTIC)):
    """(r6, r5): the largest E(six products) / E(fp32) and the smallest E(five products) / E(fp32) over kinds and sides"""
    r6, r5 = 0.0, float("inf")
    for kind in kinds:
        for side, e in emulate(t, kind).items():
            assert e["fp32"] > 0, (kind, side)
            r6 = max(r6, e["six"] / e["fp32"])
            r5 = min(r5, min(e["five"].values()) / e["fp32"])
    return r6, r5
