"""No GPU: what the host sees of the split dense sweeps' staging (csrc/mf_loss_dense.hip, the SPLIT loops of
loss_bwd_dense_kernel).  The staging changed where a tile's memory instructions are issued, not what is allocated or
launched: ``mf_loss_ws_bytes`` and ``mf_loss_plan`` of the shapes of tests/test_gpu_dense_split_stage.py are pinned here to the
values they had before.  (The side inputs are fetched as before -- four per-lane loads -- so there is no lane mapping to
restate: DESIGN 4, "Per-tile cycle budget of the split sweeps", has what was tried.)"""
from __future__ import annotations

import pytest

from tests import _dense_cases as dc

D = 128
# (B, N) -> (mf_loss_ws_bytes(B, N, 128, 4 positives, 0), (nsplit_f, tps_f, nsplit_u, tps_u, last_u, nsplit_v, tps_v, last_v))
PINNED = {
    (24, 1030): (39859456, (36, 1, 36, 1, 1, 4, 1, 1)),
    (300, 1030): (46421248, (36, 1, 36, 1, 1, 12, 1, 1)),
    (1020, 4090): (109451008, (64, 2, 64, 2, 2, 16, 2, 2)),
    (1990, 3050): (126015744, (32, 3, 32, 3, 3, 22, 3, 1)),
    (2990, 2990): (153582336, (20, 5, 20, 5, 1, 20, 5, 1)),
}


@pytest.mark.parametrize("shape", list(PINNED), ids=lambda s: f"{s[0]}x{s[1]}")
def test_workspace_and_plan_are_what_they_were(mf, shape):
    lib = mf._lib.lib()
    b, n = shape
    size, geometry = PINNED[shape]
    assert lib.mf_loss_ws_bytes(b, n, D, dc.P, 0) == size
    p = dc.plan(lib, b, n, D)
    got = tuple(p[k] for k in ("nsplit_f", "tps_f", "nsplit_u", "tps_u", "last_u", "nsplit_v", "tps_v", "last_v"))
    assert p["mined"] == 0 and got == geometry, p
