"""CPU: what the loss exports refuse, and in which words -- mf_loss_fwd / _fwd_csr / _bwd (csrc/mf_loss.hip), mf_loss_masks /
_masks_csr / mf_negative_masks (csrc/mf_loss_masks.hip), mf_mine_logits (csrc/mf_loss_mined.hip), mf_loss_plan and
mf_loss_cols_plan (host arithmetic).  The shape check the first six share is csrc/mf_loss_ws.h: loss_check_shape.

Every refusal is decided on the host before any launch, so never-dereferenced fake pointers do; every call below carries at
least one fault (or is host-only), so none reaches a launch.  The table is what the exports returned when the forward, the
backward, the masks and mf_negative_masks each restated the shape checks themselves.

Two things the table records as they are, not as one might expect: mf_loss_plan and mf_loss_cols_plan take N = 2^24 (they
launch nothing), and num_negatives = 33 at d = 256 is NOT refused by the mining check, whatever its message says about
"32 at d = 256" -- the select plan serves up to 64 at every width; the case is pinned through a workspace one byte short."""
from __future__ import annotations

import ctypes

import pytest

FAKE = ctypes.c_void_p(0x1000)
BIG = ctypes.c_size_t(2**40)
ROWC = 2                     # MF_LOSS_ROWC (include/mf_hip.h)
N24 = 1 << 24


def _args(defaults, kw):
    assert kw and set(kw) <= set(defaults), kw          # a call without a fault would be a launch
    a = dict(defaults)
    a.update(kw)
    return a


@pytest.fixture
def calls(mf):
    """name -> call(**faults) -> (code, message); the defaults of every call pass every check."""
    lib = mf._lib.lib()

    def done(rc):
        return rc, (lib.mf_last_error() if rc else b"")

    common = dict(B=4, N=1000, d=64, k=0, ws=FAKE, wsb=BIG)
    fwd_d = dict(common, P=3, sigma=1.0, margin=0.5, kinds=1 << 3, u=FAKE, v=FAKE, target=FAKE, item_idx=FAKE, pos_idx=FAKE, logq=None,
                 logq_rows=0, flags=0, out=FAKE, out_mask=None)
    csr_d = dict(fwd_d, user_ids=FAKE, pos_off=FAKE, pos_items=FAKE, num_users=10)
    del csr_d["P"], csr_d["pos_idx"]
    bwd_d = dict(common, P=3, sigma=1.0, margin=0.5, kind=3, u=FAKE, v=FAKE, flags=0, grad_out=FAKE, du=FAKE, dv=FAKE)
    masks_d = dict(common, P=3, item_idx=FAKE, pos_idx=FAKE)
    mcsr_d = dict(common, item_idx=FAKE, user_ids=FAKE, pos_off=FAKE, pos_items=FAKE, num_users=10)
    neg_d = dict(B=4, N=1000, P=3, item_idx=FAKE, pos_idx=FAKE, ws=FAKE, wsb=BIG, out=FAKE)

    def fwd(**kw):
        a = _args(fwd_d, kw)
        return done(lib.mf_loss_fwd(a["B"], a["N"], a["d"], a["P"], a["k"], a["sigma"], a["margin"], a["kinds"], a["u"], a["v"], a["target"],
                                    a["item_idx"], a["pos_idx"], a["logq"], a["logq_rows"], a["flags"], a["ws"], a["wsb"], a["out"],
                                    a["out_mask"], None))

    def fwd_csr(**kw):
        a = _args(csr_d, kw)
        return done(lib.mf_loss_fwd_csr(a["B"], a["N"], a["d"], a["k"], a["sigma"], a["margin"], a["kinds"], a["u"], a["v"], a["target"],
                                        a["item_idx"], a["user_ids"], a["pos_off"], a["pos_items"], a["num_users"], a["logq"],
                                        a["logq_rows"], a["flags"], a["ws"], a["wsb"], a["out"], a["out_mask"], None))

    def bwd(**kw):
        a = _args(bwd_d, kw)
        return done(lib.mf_loss_bwd(a["B"], a["N"], a["d"], a["P"], a["k"], a["sigma"], a["margin"], a["kind"], a["u"], a["v"], a["flags"],
                                    a["ws"], a["wsb"], a["grad_out"], a["du"], a["dv"], None))

    def masks(**kw):
        a = _args(masks_d, kw)
        return done(lib.mf_loss_masks(a["B"], a["N"], a["d"], a["P"], a["k"], a["item_idx"], a["pos_idx"], a["ws"], a["wsb"], None))

    def masks_csr(**kw):
        a = _args(mcsr_d, kw)
        return done(lib.mf_loss_masks_csr(a["B"], a["N"], a["d"], a["k"], a["item_idx"], a["user_ids"], a["pos_off"], a["pos_items"],
                                          a["num_users"], a["ws"], a["wsb"], None))

    def negative_masks(**kw):
        a = _args(neg_d, kw)
        return done(lib.mf_negative_masks(a["B"], a["N"], a["P"], a["item_idx"], a["pos_idx"], a["ws"], a["wsb"], a["out"], None))

    return dict(mf_loss_fwd=fwd, mf_loss_fwd_csr=fwd_csr, mf_loss_bwd=bwd, mf_loss_masks=masks, mf_loss_masks_csr=masks_csr,
                mf_negative_masks=negative_masks)


ITEMISED = ("mf_loss_fwd", "mf_loss_fwd_csr", "mf_loss_bwd")          # these name what is wrong with the shape
TERSE = ("mf_loss_masks", "mf_loss_masks_csr", "mf_negative_masks")   # these say "bad argument"
NULLS = {
    "mf_loss_fwd": ("u", "v", "target", "ws", "out"),
    "mf_loss_fwd_csr": ("u", "v", "target", "ws", "out"),
    "mf_loss_bwd": ("u", "v", "ws", "grad_out", "du", "dv"),
    "mf_loss_masks": ("item_idx", "ws"),
    "mf_loss_masks_csr": ("item_idx", "ws"),
    "mf_negative_masks": ("item_idx", "pos_idx", "ws", "out"),
}


def _refused(mf, calls, name, code, text, **kw):
    rc, msg = calls[name](**kw)
    assert rc == getattr(mf._lib, code) and msg.startswith(name.encode() + b": ") and text in msg, (name, kw, rc, msg)


@pytest.mark.parametrize("name", ITEMISED + TERSE)
def test_shape_and_operands(mf, calls, name):
    itemised = name in ITEMISED
    for kw in (dict(B=0), dict(B=-2), dict(B=5, N=4)):
        a = dict(dict(B=4, N=1000), **kw)
        text = b"need 0 < B <= N (B=%d N=%d)" % (a["B"], a["N"]) if itemised else b"bad argument"
        _refused(mf, calls, name, "MF_EINVAL", text, **kw)
    if name != "mf_negative_masks":                      # (it has no width: its masks are built at d = 32)
        for d in (0, 48, 512):
            _refused(mf, calls, name, "MF_EINVAL", b"embedding width %d not in {32,64,128,256}" % d if itemised else b"bad argument", d=d)
    for op in NULLS[name]:
        _refused(mf, calls, name, "MF_EINVAL", b"bad argument", **{op: None})
    _refused(mf, calls, name, "MF_ENOTSUP", b"N >= 2^24", N=N24)
    _refused(mf, calls, name, "MF_ENOTSUP", b"N >= 2^24", N=N24 + 5)


@pytest.mark.parametrize("name", ITEMISED + TERSE)
def test_workspace_one_byte_short(mf, calls, name):
    lib = mf._lib.lib()
    for k in (0, 4):
        if name == "mf_negative_masks":
            low, kw = lib.mf_negative_masks_ws_bytes(4, 1000, 3), {}
        else:
            low, kw = lib.mf_loss_ws_bytes(4, 1000, 64, 0 if name in TERSE or "fwd" in name else 3, k), dict(k=k)
        assert low > 0
        text = b"workspace too small (%d < %d)" % (low - 1, low) if name in ITEMISED else b"workspace too small"
        _refused(mf, calls, name, "MF_ENOSPC", text, wsb=ctypes.c_size_t(low - 1), **kw)
        _refused(mf, calls, name, "MF_ENOSPC", b"workspace too small", wsb=ctypes.c_size_t(0), **kw)


@pytest.mark.parametrize("name", ITEMISED)
def test_mined_limit(mf, calls, name):
    lib = mf._lib.lib()
    for k, d in ((65, 64), (65, 256), (100, 128), (999, 32)):                  # mining is on (0 < k < N) and k > 64
        _refused(mf, calls, name, "MF_ENOTSUP", b"mining with num_negatives = %d unsupported (max 64; 32 at d = 256)" % k, k=k, d=d)
    # 33 at d = 256 (and 64 anywhere) passes the mining check: the refusal that answers is the next one, the workspace's
    for k, d in ((33, 256), (64, 256), (64, 32)):
        low = lib.mf_loss_ws_bytes(4, 1000, d, 0, k)
        assert low > 0
        _refused(mf, calls, name, "MF_ENOSPC", b"workspace too small (%d < %d)" % (low - 1, low), k=k, d=d, wsb=ctypes.c_size_t(low - 1))
    # k >= N: mining is off, whatever k is -- the limit does not apply
    _refused(mf, calls, name, "MF_ENOSPC", b"workspace too small", k=1000, wsb=ctypes.c_size_t(0))


@pytest.mark.parametrize("name", ["mf_loss_fwd", "mf_loss_fwd_csr"])
def test_forward_only_refusals(mf, calls, name):
    for kinds in (0, 0x80, 0x300):
        _refused(mf, calls, name, "MF_EINVAL", b"bad argument", kinds=kinds)                       # an empty kind_mask
    _refused(mf, calls, name, "MF_EINVAL", b"MF_LOSS_ROWC needs exactly one loss kind", flags=ROWC, kinds=0b11)
    _refused(mf, calls, name, "MF_EINVAL", b"MF_LOSS_ROWC needs exactly one loss kind", flags=ROWC, kinds=0x7F)
    _refused(mf, calls, name, "MF_EINVAL", b"a logQ table needs item_idx", logq=FAKE, logq_rows=10, item_idx=None)


def test_positives(mf, calls):
    for name in ("mf_loss_fwd", "mf_loss_masks"):
        _refused(mf, calls, name, "MF_EINVAL", b"bad positives", P=-1)
        _refused(mf, calls, name, "MF_EINVAL", b"bad positives", P=3, pos_idx=None)               # P > 0 without pos_idx
    _refused(mf, calls, "mf_loss_bwd", "MF_EINVAL", b"bad argument", P=-1)
    _refused(mf, calls, "mf_negative_masks", "MF_EINVAL", b"bad argument", P=-1)
    for name in ("mf_loss_fwd_csr", "mf_loss_masks_csr"):
        _refused(mf, calls, name, "MF_EINVAL", b"pos_off is NULL", pos_off=None)
        need = b"CSR positives need user_ids, pos_off, pos_items, num_users > 0"
        for kw in (dict(num_users=0), dict(num_users=-1), dict(user_ids=None), dict(pos_items=None)):
            _refused(mf, calls, name, "MF_EINVAL", need, **kw)


def test_backward_kind(mf, calls):
    for kind in (-1, 7, 100):
        _refused(mf, calls, "mf_loss_bwd", "MF_EINVAL", b"bad argument", kind=kind)


def test_which_of_two_faults_wins(mf, calls):
    """Shape, width, operands, 2^24, the mined limit, the workspace; then what only the forward or the backward asks.  The
    masks exports look at the positives first."""
    for name in ITEMISED:
        for kw, code, text in (
            (dict(B=0, d=48), "MF_EINVAL", b"need 0 < B <= N"),
            (dict(d=48, u=None), "MF_EINVAL", b"embedding width 48"),
            (dict(u=None, N=N24), "MF_EINVAL", b"bad argument"),
            (dict(N=N24, k=65), "MF_ENOTSUP", b"N >= 2^24"),
            (dict(k=65, wsb=ctypes.c_size_t(0)), "MF_ENOTSUP", b"mining with num_negatives = 65"),
        ):
            _refused(mf, calls, name, code, text, **kw)
    for name in ("mf_loss_fwd", "mf_loss_fwd_csr"):
        _refused(mf, calls, name, "MF_ENOSPC", b"workspace too small", wsb=ctypes.c_size_t(0), out=None)
        _refused(mf, calls, name, "MF_EINVAL", b"bad argument", kinds=0, flags=ROWC)
        _refused(mf, calls, name, "MF_EINVAL", b"a logQ table needs item_idx", logq=FAKE, logq_rows=10, item_idx=None, flags=ROWC, kinds=0b11)
    _refused(mf, calls, "mf_loss_fwd", "MF_EINVAL", b"bad positives", P=-1, flags=ROWC, kinds=0b11)
    _refused(mf, calls, "mf_loss_fwd_csr", "MF_EINVAL", b"pos_off is NULL", pos_off=None, B=0)
    _refused(mf, calls, "mf_loss_bwd", "MF_ENOSPC", b"workspace too small", wsb=ctypes.c_size_t(0), kind=-1)
    _refused(mf, calls, "mf_loss_masks", "MF_EINVAL", b"bad positives", P=-1, B=0)
    _refused(mf, calls, "mf_loss_masks_csr", "MF_EINVAL", b"pos_off is NULL", pos_off=None, B=0)
    for name in TERSE:
        _refused(mf, calls, name, "MF_EINVAL", b"bad argument", ws=None, N=N24)
        _refused(mf, calls, name, "MF_ENOTSUP", b"N >= 2^24", N=N24, wsb=ctypes.c_size_t(0))
    _refused(mf, calls, "mf_loss_masks", "MF_EINVAL", b"bad argument", d=48, N=N24)


def test_mine_logits(mf):
    lib, E = mf._lib.lib(), mf._lib
    for logits, B, N, mask in ((None, 4, 8, FAKE), (FAKE, 4, 8, None), (FAKE, 0, 8, FAKE), (FAKE, -1, 8, FAKE), (FAKE, 9, 8, FAKE)):
        assert lib.mf_mine_logits(logits, B, N, 2, 1, mask, None) == E.MF_EINVAL
        assert lib.mf_last_error().startswith(b"mf_mine_logits: bad argument")
    for n in (1 << 30, (1 << 30) + 7):
        assert lib.mf_mine_logits(FAKE, 4, n, 2, 1, FAKE, None) == E.MF_ENOTSUP
        assert lib.mf_last_error().startswith(b"mf_mine_logits: N >= 2^30")
    # its limit is 2^30, not the losses' 2^24; k <= 0 or k >= N: mining disabled, nothing is launched and the mask stays
    for n, k in ((N24, 0), (N24, -3), (8, 8), (8, 100)):
        assert lib.mf_mine_logits(FAKE, 4, n, k, 1, FAKE, None) == E.MF_OK


def test_host_only_plans(mf):
    lib, E = mf._lib.lib(), mf._lib
    out = (ctypes.c_int64 * 16)()
    assert lib.mf_loss_plan(4, 1000, 64, 0, None) == E.MF_EINVAL and lib.mf_last_error() == b"mf_loss_plan: out is NULL"
    for B, N in ((0, 8), (-1, 8), (9, 8)):
        assert lib.mf_loss_plan(B, N, 64, 0, out) == E.MF_EINVAL
        assert lib.mf_last_error() == b"mf_loss_plan: need 0 < B <= N (B=%d N=%d)" % (B, N)
        assert lib.mf_loss_ws_bytes(B, N, 64, 0, 0) == 0
    assert lib.mf_loss_plan(0, 8, 48, 0, out) == E.MF_EINVAL and b"need 0 < B <= N" in lib.mf_last_error()
    assert lib.mf_loss_plan(4, 8, 48, 0, out) == E.MF_EINVAL
    assert lib.mf_last_error() == b"mf_loss_plan: embedding width 48 not in {32,64,128,256}"
    assert lib.mf_loss_plan(4, N24, 64, 0, out) == E.MF_OK                      # host arithmetic: no 2^24 limit here

    assert lib.mf_loss_cols_plan(4, 1000, 128, 10, None) == E.MF_EINVAL and lib.mf_last_error() == b"mf_loss_cols_plan: out is NULL"
    for B, N, d, ncols in ((0, 8, 128, 4), (9, 8, 128, 4), (4, 8, 128, 0), (4, 8, 128, 9), (4, 8, 48, 4)):
        assert lib.mf_loss_cols_plan(B, N, d, ncols, out) == E.MF_EINVAL
        assert lib.mf_last_error() == b"mf_loss_cols_plan: need 0 < B <= N, 1 <= ncols <= N and a supported width"
    assert lib.mf_loss_cols_plan(4, N24, 128, 10, out) == E.MF_OK
