"""CPU: the bf16-mixed precision of the transformer user tower's dense layers (*Mixed precision*).
``round_bf16`` (round-to-nearest-even on the fp32 bit pattern, held to torch), the mixed spec ``spec_tower_mixed`` /
``spec_step_mixed`` -- the plain-torch spec of tests/test_xfmr_tower_cpu.py, imported and not edited, with a rounding hook at
both operands of the six dense layers and the stated backward -- the configuration surface, the new exports, and the
rehearsal of the tower-level tolerance that tests/test_gpu_xfmr_mixed.py holds the kernels to.

The tower-level tolerance.  Rounding to bf16 is discontinuous: two fp32 evaluations that differ by accumulation order now and
then round an activation to neighbouring bf16 values (a relative step of 2^-8 on that element), so one sample of "the fp32
spec's own error" may or may not contain such flips.  The rule is therefore: per shape, E = the LARGEST over ``SEEDS`` worlds
of the mixed spec in fp32 against the mixed spec in fp64, per tensor, max-abs over max-abs; the thing under test is held, on
each of those worlds, to 8 E + 1e-7.  That only means something if EVERY sample contains flips, which is a matter of how many
activations a world rounds: with the eight lists of the fp32 tower's tests and L = 7 (about 45 tokens) the per-seed errors of
u at d = 32 were all ~1.5e-7 (no flip in eight worlds) while gradients showed 3e-5 on two seeds and 1e-7 on the others, and
with "cls" pooling (only position 0 reaches u) the bias gradients' E came out 20 x smaller than their neighbours'.  Such worlds
are enlarged (``WORLD_REPEATS``: the same list sizes, drawn that many times over) until every seed's error is of one order;
the factor stays 8.  Here the thing under test is a stand-in for the kernels: the fp32 mixed spec whose dense
layers accumulate in k-blocks of 16, sequentially.  Every figure is printed before it is asserted (``pytest -s``)."""
from __future__ import annotations

import contextlib
import ctypes
import functools
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_xfmr_tower import _lists, _world
from tests.test_xfmr_dropout_cpu import spec_step_dropout
from tests.test_xfmr_tower_cpu import HARD_CASES, hard_case, rel_err, spec_step, spec_tower

_LINEAR = F.linear


# ---------------------------------------------------------------------------------------- the rounding ----
def round_bf16(x) -> np.ndarray:
    """fp32 -> the nearest bf16 (ties to even), as fp32: add 0x7FFF + the kept lsb to the bit pattern, clear the low half.
    (Sign-magnitude: the same on negatives; subnormals are ordinary bit patterns.  No NaN handling.)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return r.astype(np.uint32).view(np.float32)


def trunc_bf16(x) -> np.ndarray:
    """fp32 -> bf16 by dropping the low half (round toward zero): what the GPU tests show the kernels do NOT do."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def rnd_torch(t: torch.Tensor) -> torch.Tensor:
    """The rounding hook of the spec: the nearest bf16 of every element, in the tensor's own dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def identity(t: torch.Tensor) -> torch.Tensor:
    return t


def mm_blocks16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a @ b accumulated in k-blocks of 16, block after block: the order of a 16-deep MFMA chain, not of a BLAS."""
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=a.dtype)
    for k in range(0, a.shape[1], 16):
        acc = acc + a[:, k:k + 16] @ b[k:k + 16]
    return acc


class _MixedLinear(torch.autograd.Function):
    """Y = rnd(X) rnd(W)^T + b; dX = rnd(dY) rnd(W), dW = rnd(dY)^T rnd(X), db = the column sums of the UNROUNDED dY."""

    @staticmethod
    def forward(ctx, x, w, b, rnd, mm):
        xr, wr = rnd(x), rnd(w)
        ctx.save_for_backward(xr, wr)
        ctx.rnd, ctx.mm = rnd, mm
        return _LINEAR(xr, wr, b) if mm is None else mm(xr, wr.t()) + b

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        mm = ctx.mm or torch.mm
        dyr = ctx.rnd(dy)
        return mm(dyr, wr), mm(dyr.t(), xr), dy.sum(0), None, None


@contextlib.contextmanager
def mixed_dense(rnd=rnd_torch, mm=None):
    """Inside: every ``F.linear`` -- in the imported specs exactly the six dense layers of an encoder layer -- is the mixed one."""
    with mock.patch.object(F, "linear", lambda x, w, b=None: _MixedLinear.apply(x, w, b, rnd, mm)):
        yield


def spec_tower_mixed(w, lists, sd, *, rnd=rnd_torch, mm=None, **kw):
    with mixed_dense(rnd, mm):
        return spec_tower(w, lists, sd, **kw)


def spec_step_mixed(w, sd, lists, c, kw, extra, lr, dtype, *, rnd=rnd_torch, mm=None):
    with mixed_dense(rnd, mm):
        return spec_step(w, sd, lists, c, kw, extra, lr, dtype)


def spec_step_dropout_mixed(w, sd, lists, c, kw, extra, lr, dtype, drop, *, rnd=rnd_torch, mm=None):
    """``spec_step_dropout`` (``spec_tower_dropout`` with its numpy masks) with the rounding hook added."""
    with mixed_dense(rnd, mm):
        return spec_step_dropout(w, sd, lists, c, kw, extra, lr, dtype, drop)


# ------------------------------------------------------------------------------ the tower-level worlds ----
# (d, heads, L, mode, layers, act, intermediate): d in {32, 64, 128}; head widths 8, 16, 32, 64 once each; L in {7, 64}; 1 and
# 2 layers; I in {32, 96, 512} (512 needs d = 128; 96 < 128 is the I < h case); the three pooling modes; the four activations
TOWER_CASES = [(32, 4, 7, "mean", 1, "gelu", 32), (64, 4, 64, "max", 2, "relu", 96), (128, 4, 64, "cls", 1, "silu", 512),
               (128, 2, 7, "mean", 2, "gelu_new", 96)]
DROPOUT_CASE = (64, 4, 16, "mean", 2, "gelu", 64)
DROPOUT = {"p_hidden": 0.1, "p_attn": 0.1, "seed": 20240611, "call": 0}
SEEDS = tuple(range(8))
ROWS = 300
SIZES = [1, 5, 17, 64, 65, 130, 3, 9]
WORLD_REPEATS = {7: 8, 16: 4, 64: 1, "cls": 4}      # by L (tokens per list), and for "cls" pooling: see the module docstring
LR = 0.5
FACTOR = 8.0


def tower_world(case, seed):
    """(w, sd, lists, c, extra, kw) of one seed of one case, fp64."""
    d, heads, L, mode, layers, act, inter = case
    w, sd = _world(1000 * seed + d + heads + L, ROWS, d, layers, inter, 64)
    lists = _lists(np.random.default_rng(100 * seed + d + L), ROWS, SIZES * max(WORLD_REPEATS[L], WORLD_REPEATS.get(mode, 1)))
    g = torch.Generator().manual_seed(10 * seed + d)
    c = torch.randn(len(lists), d, generator=g, dtype=torch.float64)
    extra = (torch.randint(0, ROWS, (40,), generator=g), torch.randn(40, d, generator=g, dtype=torch.float64))
    kw = {"heads": heads, "act": act, "mode": mode, "n_i": True, "n_u": True, "max_history": L}
    return w, sd, lists, c, extra, kw


def _step(case, seed, dtype, drop, mm=None):
    w, sd, lists, c, extra, kw = tower_world(case, seed)
    if drop is None:
        return spec_step_mixed(w, sd, lists, c, kw, extra, LR, dtype, mm=mm)
    return spec_step_dropout_mixed(w, sd, lists, c, kw, extra, LR, dtype, drop, mm=mm)


def flatten(step) -> dict:
    """{tensor name: tensor} of a (u, table delta, dense gradients) triple."""
    u, delta, grads = step
    return {"u": u, "table step": delta, **grads}


@functools.lru_cache(maxsize=None)
def reference(case, dropout: bool = False):
    """(per seed: the fp64 mixed spec's tensors; E: per tensor, the largest fp32-against-fp64 error of the mixed spec over
    SEEDS).  Computed once per case and shared (tests must not modify it)."""
    drop = DROPOUT if dropout else None
    ref64 = [flatten(_step(case, s, torch.float64, drop)) for s in SEEDS]
    e = {k: 0.0 for k in ref64[0]}
    for s in SEEDS:
        f32 = flatten(_step(case, s, torch.float32, drop))
        for k in e:
            e[k] = max(e[k], rel_err(f32[k], ref64[s][k]))
    return ref64, e


def family(name: str) -> str:
    """The row of DESIGN's table that a tensor belongs to."""
    if name in ("u", "table step"):
        return name
    if "LayerNorm" in name:
        return "LayerNorm gradients"
    if name.startswith("embeddings."):
        return "position / token-type gradients"
    return "dense weight gradients" if name.endswith(".weight") else "dense bias gradients"


def hold(label: str, got: dict, ref: dict, e: dict, worst: dict | None = None) -> None:
    """The rule: per tensor, rel_err(got, fp64 mixed spec) <= 8 E + 1e-7; prints every figure first, then asserts them all."""
    bad = []
    for k in ref:
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), (label, k)
        err = rel_err(got[k].cpu(), ref[k])
        ratio = err / e[k] if e[k] > 0 else (0.0 if err == 0 else float("inf"))
        print(f"  {label} {k}: error {err:.3e}  E {e[k]:.3e}  ratio {ratio:.2f}")
        if worst is not None:
            worst[family(k)] = max(worst.get(family(k), 0.0), ratio)
        if not err <= FACTOR * e[k] + 1e-7:
            bad.append((k, err, e[k]))
    assert not bad, (label, bad)


# --------------------------------------------------------------------------------------------- tests ----
def test_round_bf16_is_torchs_rounding():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1 << 16, generator=g) * torch.tensor(10.0) ** torch.randint(-30, 30, (1 << 16,), generator=g)
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0])
    tiny = torch.tensor([2.0 ** -133, -(2.0 ** -133), 3 * 2.0 ** -134, 2.0 ** -126 * (1 + 2.0 ** -8), 2.0 ** -134, -(2.0 ** -134),
                         5 * 2.0 ** -135, 2.0 ** -140])                      # bf16 subnormals (below 2^-126) and ties among them
    for t in (x, -x.abs(), ties, tiny, x * 2.0 ** -120):
        want = t.bfloat16().float().numpy()
        got = round_bf16(t.numpy())
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert round_bf16(np.float32(1 + 2.0 ** -8)) == 1.0 and round_bf16(np.float32(1 + 3 * 2.0 ** -8)) == 1 + 2.0 ** -6
    assert trunc_bf16(np.float32(1 + 3 * 2.0 ** -8)) == 1 + 2.0 ** -7
    assert torch.equal(rnd_torch(x.double()), x.bfloat16().double())


@pytest.mark.parametrize("case", HARD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_identity_hook_is_the_plain_spec(case):
    w, sd, lists, c, kw = hard_case(*case)
    w32, sd32 = w.float(), {k: v.float() for k, v in sd.items()}
    with torch.no_grad():
        want = spec_tower(w32, lists, sd32, **kw)
        assert torch.equal(spec_tower_mixed(w32, lists, sd32, rnd=identity, **kw), want)
        got = spec_tower_mixed(w32, lists, sd32, **kw)
    moved = rel_err(got, want)
    print(f"  rounding moves u by {moved:.3e}")
    assert 1e-4 < moved < 5e-2                                               # noqa: PLR2004  (the hook is live, and sane)


def test_mixed_backward_is_the_stated_one():
    """dY is rounded for dX and dW, not for db; X and W are the rounded ones."""
    g = torch.Generator().manual_seed(3)
    x, w, b = (torch.randn(s, generator=g, dtype=torch.float64).requires_grad_(True) for s in ((9, 32), (48, 32), (48,)))
    dy = torch.randn(9, 48, generator=g, dtype=torch.float64)
    with mixed_dense():
        y = F.linear(x, w, b)
    y.backward(dy)
    r = rnd_torch
    assert torch.equal(y.detach(), r(x.detach()) @ r(w.detach()).t() + b.detach())
    assert torch.equal(x.grad, r(dy) @ r(w.detach())) and torch.equal(w.grad, r(dy).t() @ r(x.detach()))
    assert torch.equal(b.grad, dy.sum(0)) and not torch.equal(b.grad, r(dy).sum(0))
    assert F.linear is _LINEAR                                               # the hook is gone outside the context


def test_config_surface(mf):
    models = mf.models
    assert models.ModelConfig().precision == "fp32" and models.PRECISIONS == ("fp32", "bf16-mixed")
    cfg = models.ModelConfig(user_tower="transformer", precision="bf16-mixed")
    assert cfg.precision == "bf16-mixed"
    for tower in ("table", "history", "features"):
        with pytest.raises(ValueError, match="precision"):
            models.ModelConfig(user_tower=tower, precision="bf16-mixed")
        assert models.ModelConfig(user_tower=tower, precision="fp32").precision == "fp32"
    for bad in ("fp16", "bf16"):
        with pytest.raises(ValueError):
            models.ModelConfig(user_tower="transformer", precision=bad)
        with pytest.raises(ValueError, match="fp32.*bf16-mixed"):
            models.check_precision(bad)
    lit = mf.lightning.MatrixFactorizationLitConfig(user_tower="transformer", precision="bf16-mixed", hidden_size=32)
    assert lit.precision == "bf16-mixed"
    again = mf.lightning.MatrixFactorizationLitConfig(**lit.model_dump())
    assert again.precision == "bf16-mixed" and again == lit
    assert mf.lightning.MatrixFactorizationLitConfig().model_dump()["precision"] == "fp32"


def test_tower_carries_the_precision(mf):
    models = mf.models
    item = models.EmbeddingTower(50, 32, device="cpu")
    plain = models.HistoryTransformerTower(item)
    mixed = models.HistoryTransformerTower(item, precision="bf16-mixed")
    assert plain.precision == "fp32" and mixed.precision == "bf16-mixed"
    assert "precision" not in plain.extra_repr() and "precision=bf16-mixed" in mixed.extra_repr()
    assert list(plain.state_dict()) == list(mixed.state_dict())             # the names are BertModel's, unchanged
    for bad in ("fp16", "bf16"):
        with pytest.raises(ValueError, match="precision"):
            models.HistoryTransformerTower(item, precision=bad)
    towers = models.init_towers(models.ModelConfig(num_users=10, num_items=50, hidden_size=32, user_tower="transformer",
                                                   precision="bf16-mixed"), device="cpu")
    assert towers["user"].precision == "bf16-mixed"


def test_abi(mf):
    lib = mf._lib.lib()
    header = (mf._lib._PKG.parent / "include" / "mf_hip.h").read_text()
    for name in ("mf_xfmr_forward_mixed", "mf_xfmr_backward_mixed", "mf_xfmr_dense", "mf_xfmr_dense_ws_bytes"):
        assert name in mf._lib.SIGNATURES and f"{name}(" in header and getattr(lib, name) is not None
    assert "#define MF_XFMR_FP32 0" in header and "#define MF_XFMR_BF16_MIXED 1" in header
    assert (mf._lib.XFMR_FP32, mf._lib.XFMR_BF16_MIXED) == (0, 1)
    # the argument checks come before any GPU call: an unknown precision or form is refused on a machine without a GPU
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    assert lib.mf_xfmr_dense(0, 7, 4, 32, 32, p, p, None, p, None, p, 16384, None) == mf._lib.MF_EINVAL
    assert b"precision 7" in lib.mf_last_error()
    assert lib.mf_xfmr_dense(3, 1, 4, 32, 32, p, p, None, p, None, p, 16384, None) == mf._lib.MF_EINVAL
    assert b"form 3" in lib.mf_last_error()
    assert lib.mf_xfmr_dense(0, 1, 4, 48, 32, p, p, None, p, None, p, 16384, None) == mf._lib.MF_ENOTSUP
    # workspaces: the token count, and for the weight gradient 256 slices of [N, K] + [N] partials
    assert lib.mf_xfmr_dense_ws_bytes(0, 64, 128) == lib.mf_xfmr_dense_ws_bytes(1, 64, 128) > 0
    assert lib.mf_xfmr_dense_ws_bytes(2, 64, 128) >= 256 * (64 * 128 + 64) * 4
    assert lib.mf_xfmr_dense_ws_bytes(3, 64, 128) == 0 and lib.mf_xfmr_dense_ws_bytes(0, 48, 128) == 0
    # the existing workspace exports keep their values: the mixed mode adds nothing to the stash or the backward workspace
    assert lib.mf_xfmr_backward_dropout_ws_bytes(1000, 64, 96) - lib.mf_xfmr_backward_ws_bytes(1000, 64, 96) >= 1000 * 64 * 4


@pytest.mark.parametrize("case", TOWER_CASES + [DROPOUT_CASE], ids=lambda c: "-".join(map(str, c)))
def test_tolerance_rehearsal(case):
    """The stand-in (fp32 mixed spec, dense layers accumulated in k-blocks of 16) passes the rule of the module docstring on
    every seed of every shape that the GPU tests use."""
    dropout = case is DROPOUT_CASE
    ref64, e = reference(case, dropout)
    for s in SEEDS:
        got = flatten(_step(case, s, torch.float32, DROPOUT if dropout else None, mm=mm_blocks16))
        hold(f"seed {s}", got, ref64[s], e)
