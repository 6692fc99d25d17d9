"""GPU: the split-bf16 mining prefilter (csrc/mf_mine_bf.h) at the batch sizes it serves by default (B >= 4096) and
beyond, where its plan has few item chunks (nchunk < 16), four rescoring lanes per chunk (num_negatives > 16) and copy
bitmaps of more than 256 columns a bit.  Every case reads the prefilter's counters (mf_probe_mining_prefilter) to
show WHICH search answered: a prefilter that gives up hands the batch to the fp32 search on the device, and a "mode 1
equals mode 0" comparison would then check nothing.  Bars: the mined masks, the loss and both gradients bit-identical
to the fp32 search (mode 0); sampled users' masks bit-exact against the oracle; the loss within
``gu.loss_tolerance`` of an fp64 restatement built from the same mask, sampled dU rows within ``gu.assert_grads_close``."""
from __future__ import annotations

import ctypes

import pytest
import torch

from oracle import chain, losses as ol
from tests import _golden_util as gu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1.0
NUM_ITEMS = 62_423                       # MovieLens-sized id space, Zipf(1) popularity (as bench.py draws its batches)


def _plan(lib, b, n, d, k):
    out = (ctypes.c_int64 * 8)()
    assert lib.mf_mining_prefilter_plan(b, n, d, k, out) == 0
    return dict(zip(("ok", "pays", "nchunk", "tpc", "lpc", "nlists", "keys_cap", "lds"), list(out)))


def _counters(lib):
    """[0] candidates rescored, [1] users rescored, [2] users walked exactly, [3] users without a bound, [4] non-finite
    inputs, [5] zero targets, [6] entries spilled, [8] the longest copy-expansion pool -- since the last call; resets them."""
    buf = (ctypes.c_ulonglong * 16)()
    assert lib.mf_probe_mining_prefilter(buf, 1) == 0
    return list(buf)


def _answered_by(c, b):
    if c[1] or c[2]:
        assert c[1] + c[2] == b and c[3] == 0 and c[4] == 0, str(c)
        return "prefilter"
    assert c[1] == 0 and c[2] == 0, str(c)
    return "fp32"


def _run(mf, case, kind, k, sigma, mode):
    """The mined loss through mf.losses with the candidate search in `mode`: (mask on the device, loss, dU, dV, counters)."""
    lib = mf._lib.lib()
    b = case["u"].shape[0]
    kw = dict(item_idx=case["item_idx"], pos_idx=case["pos_idx"], logq_table=case["logq_table"])
    try:
        lib.mf_set_mining_prefilter(mode)
        _counters(lib)
        mask = mf.losses.negative_mask(case["u"], case["v"], case["target"], num_negatives=k, sigma=sigma, **kw)
        c_mask = _counters(lib)
        u, v = case["u"].clone().requires_grad_(), case["v"].clone().requires_grad_()
        loss = getattr(mf.losses, kind)(num_negatives=k, sigma=sigma, margin=MARGIN)(u, v, case["target"], **kw)
        loss.backward()
        c = _counters(lib)
    finally:
        lib.mf_probe_mining_prefilter(None, 0)
        lib.mf_set_mining_prefilter(1)
    assert _answered_by(c_mask, b) == _answered_by(c, b), (c_mask, c)      # (the same search on the same inputs)
    return mask, loss.detach(), u.grad, v.grad, c


def _rows_loss64(kind, case, rows, m_rows, sigma, u_rows=None):
    """fp64 per-user terms of the users `rows` (their own columns are their diagonals), from the given mined mask rows."""
    u = case["u"][rows].double() if u_rows is None else u_rows
    v = case["v"].double()
    t = case["target"][rows].double()
    lq = case["logq_table"].double()[case["item_idx"]]
    sq = ((u * u).sum(-1)[:, None] + (v * v).sum(-1)[None, :] - 2.0 * (u @ v.T)).clamp_min(0.0)
    lg = -0.5 * sq * torch.sign(t)[:, None] * sigma - lq[None, :]
    at = torch.arange(rows.numel(), device=lg.device)
    diag = lg[at, rows]
    if kind == "PairwiseHingeLoss":
        x = torch.relu(lg - diag[:, None] + MARGIN)
        wm = m_rows.double()
        per = (x * wm / (wm.sum(-1, keepdim=True) + 1e-10)).sum(-1)
    else:
        assert kind == "InfomationNoiseContrastiveEstimationLoss", kind
        mm = m_rows.clone()
        mm[at, rows] = True
        per = torch.logsumexp(torch.where(mm, lg, torch.full_like(lg, float("-inf"))), dim=-1) - diag
    return per * t.abs()


def _check_oracle(case, mask, k, sigma, n_rows, seed):
    """`n_rows` sampled users' mined masks, bit for bit, against the oracle's chain logits and semi-hard mining."""
    b = case["u"].shape[0]
    rows = torch.randperm(b, generator=torch.Generator().manual_seed(seed))[:n_rows].sort().values
    item_idx, pos_idx = case["item_idx"].cpu(), case["pos_idx"].cpu()
    lq = case["logq_table"].cpu()[item_idx]
    lg = torch.from_numpy(chain.logits(case["u"].cpu()[rows].numpy(), case["v"].cpu().numpy(), case["target"].cpu()[rows].numpy(),
                                       sigma, lq.numpy()))
    neg = ol.negative_masks(item_idx, pos_idx, b, rows=rows)
    want = ol.semi_hard_mining(lg, neg, k, diag=lg[torch.arange(rows.numel()), rows])
    got = mask[rows.to(DEV)].cpu()
    bad = (got != want).any(1).nonzero().flatten()
    assert not bad.numel(), ("rows differ from the oracle", rows[bad][:8].tolist())
    return rows


def _zipf_case(b, n, d, seed):
    """A bench-shaped batch: item rows looked up by id in a unit-row table (Zipf(1) ids for the users' positives, uniform
    ids behind them: hundreds of exact copies of the popular items), a logQ table over the ids, targets in -2..5 (zero
    and negative ones included), six positives per user of which every fifth user's own is missing."""
    g = torch.Generator().manual_seed(seed)
    zipf = 1.0 / torch.arange(1, NUM_ITEMS, dtype=torch.float64)
    ids = torch.cat([torch.multinomial(zipf, b, replacement=True, generator=g) + 1, torch.randint(1, NUM_ITEMS, (n - b,), generator=g)])
    table = torch.nn.functional.normalize(torch.randn(NUM_ITEMS, d, generator=g), dim=-1)
    pos = torch.multinomial(zipf, b * 6, replacement=True, generator=g).reshape(b, 6) + 1
    pos[:, 0] = ids[:b]
    pos[::5, 0] = 0                                              # (0 = padding: no item carries it)
    case = {
        "u": torch.nn.functional.normalize(torch.randn(b, d, generator=g), dim=-1),
        "v": table[ids],
        "target": torch.randint(-2, 6, (b,), generator=g),
        "item_idx": ids,
        "pos_idx": pos,
        "logq_table": torch.log(zipf / zipf.sum()).float(),
    }
    case["logq_table"] = torch.cat([torch.zeros(1), case["logq_table"]])      # indexed by id (id 0: padding)
    assert int(torch.bincount(ids).max()) >= 200                               # (the copies are there)
    return case


def _to_dev(case):
    return {name: x.to(DEV) for name, x in case.items()}


DEFAULT_CASES = [(4100, 8200, 64, 4, 1.0), (8192, 16384, 128, 4, 1.0), (8192, 16384, 128, 16, 30.0), (8192, 16384, 128, 32, 1000.0)]


@pytest.mark.parametrize("cfg", DEFAULT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_default_mode_is_the_fp32_search_at_the_batch_sizes_it_serves(mf, cfg):
    """Mode 1 (no forcing) at B >= 4096: the prefilter answers (the counters say so), and its masks, loss, dU and dV are
    the fp32 search's bits; 64 users' masks are the oracle's; the loss and sampled dU rows match an fp64 restatement.
    B = 4100 pads the last user block and leaves a ragged last item tile."""
    b, n, d, k, sigma = cfg
    lib = mf._lib.lib()
    plan = _plan(lib, b, n, d, k)
    assert plan["ok"] and plan["pays"], plan
    case = _to_dev(_zipf_case(b, n, d, seed=b + d + k))
    kinds = ["PairwiseHingeLoss"] + (["InfomationNoiseContrastiveEstimationLoss"] if k == 16 else [])
    for kind in kinds:
        m1, l1, du1, dv1, c1 = _run(mf, case, kind, k, sigma, mode=1)
        m0, l0, du0, dv0, c0 = _run(mf, case, kind, k, sigma, mode=0)
        assert _answered_by(c1, b) == "prefilter" and _answered_by(c0, b) == "fp32", (c1, c0)
        assert torch.equal(m1, m0), int((m1 != m0).sum())
        assert torch.equal(l1, l0) and torch.equal(du1, du0) and torch.equal(dv1, dv0), (kind, float(l1), float(l0))
        rows = _check_oracle(case, m1, k, sigma, 64, seed=k)
        # the loss: a plain sum of per-user terms -- the whole batch in fp64 from the same mask, in blocks of users
        t = case["target"].cpu().numpy()
        want = 0.0
        for r0 in range(0, b, 1024):
            r = torch.arange(r0, min(b, r0 + 1024), device=DEV)
            want += float(_rows_loss64(kind, case, r, m1[r], sigma).sum())
        assert abs(float(l1) - want) <= gu.loss_tolerance(want, sigma, t), (kind, float(l1), want)
        # dU of a user depends on its own term only: the sampled rows' fp64 gradients are exact references
        rd = rows.to(DEV)
        ur = case["u"][rd].double().requires_grad_()
        _rows_loss64(kind, case, rd, m1[rd], sigma, u_rows=ur).sum().backward()
        gu.assert_grads_close(du1[rd].cpu().numpy(), ur.grad.cpu().numpy(), sigma, (kind, "du"))


def _copy_heavy_case(b, n, d, seed):
    """Every column from 48 item ids (tens to hundreds of copies each), every item row the same unit vector, the order
    decided by the logQ table alone: ids 1..24 at -2, ids 25..48 at -1 -- so within each half every column ties EXACTLY
    with every other, different ids included, and ties go to the lower column.  The first half of the columns carries
    ids 25..48 (columns 0..23 in order, 24..47 in reverse order, then random ones), the second half ids 1..24.  For a
    user whose own id is in 1..24 the ids 25..48 are semi-hard at Dm = -1 and come first; for the others they are the
    first hard ones at Dm = 0.  Either way ~24 representatives per item chunk pass the scan (the scan's hit buffer holds
    32 per user and chunk), the k = 32 winners are the 24 of columns 0..23 and eight more, the copy-expansion pool holds
    the k winners and k - 1 - t copies behind the winner at position t (528 keys), and the selected columns are the
    representatives 0..23 and columns 24..31: the FIRST copies of the LAST winners, written near the end of the pool."""
    g = torch.Generator().manual_seed(seed)
    h = n // 2
    ids = torch.cat([torch.randint(25, 49, (h,), generator=g), torch.randint(1, 25, (n - h,), generator=g)])
    ids[:24] = torch.arange(25, 49)
    ids[24:48] = torch.arange(48, 24, -1)
    ids[h:h + 24] = torch.arange(1, 25)
    w = torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=-1)
    logq = torch.zeros(49)
    logq[1:25], logq[25:] = -2.0, -1.0
    pos = torch.stack([ids[:b], torch.randint(1, 49, (b,), generator=g)], dim=1)
    pos[::5, 0] = 0
    assert int(torch.bincount(ids)[1:].min()) >= 32
    return {
        "u": torch.nn.functional.normalize(torch.randn(b, d, generator=g), dim=-1),
        "v": w.expand(n, d).clone(),
        "target": torch.randint(-2, 6, (b,), generator=g),
        "item_idx": ids,
        "pos_idx": pos,
        "logq_table": logq,
    }


FEW_CHUNKS = [((16384, 16384, 128, 32, 1.0), 8), ((32768, 32768, 64, 32, 1.0), 4), ((65536, 65536, 64, 24, 1.0), 2),
              ((65536, 65536, 64, 32, 1.0), 2)]


@pytest.mark.parametrize("cfg,nchunk", FEW_CHUNKS, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_few_item_chunks_and_a_full_copy_pool_equal_the_fp32_search(mf, cfg, nchunk):
    """Mode 2 against mode 0 where the plan has few item chunks (B > 8192) and four rescoring lanes per chunk: the
    rescoring wave's key array was shortest there (16 nlists + 136 keys: 264 at two chunks), and the copy-expansion pool
    is longest.  The counters show the prefilter served the batch and how long the longest pool was: past the old
    capacity at 4 and 2 chunks, and at two chunks and k = 32 past where the old LDS allocation ended (its win / sorted /
    row words behind the keys) -- the selected copies of the last winners were written there, and lost.  Masks compared
    on the device (65,536^2 bools: 4.3 GB), loss, dU and dV bit for bit; 32 users against the oracle."""
    b, n, d, k, sigma = cfg
    lib = mf._lib.lib()
    plan = _plan(lib, b, n, d, k)
    assert plan["ok"] and plan["nchunk"] == nchunk and plan["lpc"] == 4, plan
    assert plan["keys_cap"] >= k * (k + 1) // 2, plan
    case = _to_dev(_copy_heavy_case(b, n, d, seed=b + k))
    m2, l2, du2, dv2, c2 = _run(mf, case, "PairwiseHingeLoss", k, sigma, mode=2)
    assert _answered_by(c2, b) == "prefilter", str(c2)
    old_cap = 16 * plan["nlists"] + 136                      # keys[] before it took k into account
    old_room = old_cap + (2 * 64 * 8 + d * 4) // 8            # ... and the old allocation's words behind it
    pool = c2[8]
    assert pool >= 0.8 * k * (k + 1) // 2 and pool <= k * (k + 1) // 2, str(c2)
    if k * (k + 1) // 2 > old_cap:
        assert pool > old_cap, (pool, old_cap)
    if nchunk == 2 and k == 32:
        assert pool > old_room, (pool, old_room)
    m0, l0, du0, dv0, c0 = _run(mf, case, "PairwiseHingeLoss", k, sigma, mode=0)
    assert _answered_by(c0, b) == "fp32", c0
    assert torch.equal(m2, m0), int((m2 != m0).sum())
    del m0
    assert torch.equal(l2, l0) and torch.equal(du2, du0) and torch.equal(dv2, dv0), (float(l2), float(l0))
    _check_oracle(case, m2, k, sigma, 32, seed=k)


def test_the_prefilter_gives_up_at_full_size_and_the_fp32_search_answers(mf):
    """A thousand bit-identical item rows under DIFFERENT ids (nothing marks them as copies) at the cut of a user:
    a thousand exact ties overflow its lists and its spill list, the device gate hands the batch to the fp32 search
    (the counters show no user answered by the prefilter), and every output is mode 0's."""
    b, n, d, k, sigma = 8192, 16384, 128, 4, 1.0
    lib = mf._lib.lib()
    assert _plan(lib, b, n, d, k)["pays"]
    case = _zipf_case(b, n, d, seed=3)
    case["target"][0] = 3
    # user 0's best negative (the oracle, k = 1), copied under a thousand fresh ids with its logQ
    lq = case["logq_table"][case["item_idx"]]
    lg = torch.from_numpy(chain.logits(case["u"][:1].numpy(), case["v"].numpy(), case["target"][:1].numpy(), sigma, lq.numpy()))
    best = int(ol.semi_hard_mining(lg, ol.negative_masks(case["item_idx"], case["pos_idx"], b, rows=torch.tensor([0])), 1,
                                   diag=lg[:, 0]).nonzero()[0, 1])
    at = torch.arange(n // 2, n // 2 + 1000)
    assert best not in at.tolist() and best != 0
    fresh = NUM_ITEMS + torch.arange(1000)                      # (the table grows by these rows below)
    case["v"][at] = case["v"][best].clone()
    case["item_idx"][at] = fresh
    case["logq_table"] = torch.cat([case["logq_table"], torch.full((1000,), float(case["logq_table"][case["item_idx"][best]]))])
    # every valid column tied with it bit for bit (the thousand, and copies of its item under its own id)
    neg0 = ol.negative_masks(case["item_idx"], case["pos_idx"], b, rows=torch.tensor([0]))[0]
    lq = case["logq_table"][case["item_idx"]]
    ties = ((case["v"] == case["v"][best]).all(1) & (lq == lq[best]) & neg0).nonzero().flatten().tolist()
    assert len(ties) >= 1001, len(ties)
    case = _to_dev(case)
    m1, l1, du1, dv1, c1 = _run(mf, case, "PairwiseHingeLoss", k, sigma, mode=1)
    assert _answered_by(c1, b) == "fp32" and c1[6] > 0, c1                   # (the prefilter ran, spilled, and gave up)
    m0, l0, du0, dv0, _ = _run(mf, case, "PairwiseHingeLoss", k, sigma, mode=0)
    assert torch.equal(m1, m0) and torch.equal(l1, l0) and torch.equal(du1, du0) and torch.equal(dv1, dv0)
    # user 0 mined the lowest columns of its exact ties: the construction hit its cut
    assert m1[0].nonzero().flatten().tolist() == ties[:k]
