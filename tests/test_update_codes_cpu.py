"""CPU: the return code of a sparse row update export when a call has TWO faults at once -- the order of the host-side
checks.  The single-table exports ask bad argument -> table too large -> width -> workspace -> (n == 0: nothing to do); the
pair exports ask bad argument -> width -> table too large -> list lengths -> workspace; Adam's step and Adagrad's
hyper-parameters come before all of these.  Every pointer is a fake non-null one: each refusal is decided before any launch."""
from __future__ import annotations

import ctypes

import pytest

FAKE = ctypes.c_void_p(0x1000)
BIG = 1 << 39


def _ws(lib, n, d):
    return lib.mf_update_ws_bytes(max(n, 1), d)


def _sgd(lib, *, d=32, n_rows=100, n=4, ws=FAKE, short=0):
    return lib.mf_update_sgd(FAKE, n_rows, d, FAKE, n, FAKE, 0, 0.05, 0.0, ws, _ws(lib, n, d) - short, None)


def _adam(lib, *, table=FAKE, step=1):
    return lib.mf_update_adam(table, FAKE, FAKE, 100, 32, FAKE, 4, FAKE, 0, step, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, FAKE, _ws(lib, 4, 32),
                              None)


def _adagrad(lib, *, table=FAKE, eps=1e-10):
    return lib.mf_update_adagrad(table, FAKE, 100, 32, FAKE, 4, FAKE, 0, 0.05, eps, 0.0, FAKE, _ws(lib, 4, 32), None)


def _pair(lib, adam, *, d=32, n_rows_a=100, n_a=4, short_b=0):
    dw = d if d in (32, 64, 128, 256) else 32
    return lib.mf_update_pair(adam, d, FAKE, FAKE, FAKE, n_rows_a, FAKE, n_a, FAKE, 0, FAKE, _ws(lib, n_a, dw), FAKE, FAKE, FAKE, 100, FAKE, 4,
                              FAKE, 0, FAKE, _ws(lib, 4, dw) - short_b, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, None)


def _pair_adagrad(lib, *, d=32, n_rows_a=100, n_a=4, short_b=0):
    dw = d if d in (32, 64, 128, 256) else 32
    return lib.mf_update_pair_adagrad(d, FAKE, FAKE, n_rows_a, FAKE, n_a, FAKE, 0, FAKE, _ws(lib, n_a, dw), FAKE, FAKE, 100, FAKE, 4, FAKE, 0,
                                      FAKE, _ws(lib, 4, dw) - short_b, 0.05, 1e-10, 0.0, None)


def _refused(lib, rc, want, export, *words):
    msg = lib.mf_last_error().decode()
    assert rc == want, (export, rc, msg)
    assert msg.startswith(export + ":"), msg                     # every message begins with its export's name
    for w in words:
        assert w in msg, (w, msg)


def test_single_table_exports_with_two_faults(mf):
    lib, L = mf._lib.lib(), mf._lib
    _refused(lib, _sgd(lib, d=48, n_rows=BIG), L.MF_ENOTSUP, "mf_update_sgd", "too large")          # the table's size before the width
    _refused(lib, _sgd(lib, d=48, short=1), L.MF_EINVAL, "mf_update_sgd", "width")                   # the width before the workspace
    _refused(lib, _sgd(lib, n=0, ws=None), L.MF_EINVAL, "mf_update_sgd", "bad argument")             # the arguments before "nothing to do"
    _refused(lib, _adam(lib, step=0, table=None), L.MF_EINVAL, "mf_update_adam", "step")             # Adam's step before everything
    _refused(lib, _adagrad(lib, eps=0.0, table=None), L.MF_EINVAL, "mf_update_adagrad", "eps")       # Adagrad's hyper-parameters too


@pytest.mark.parametrize("export", ["mf_update_pair:sgd", "mf_update_pair:adam", "mf_update_pair_adagrad"])
def test_pair_exports_with_two_faults(mf, export):
    lib, L = mf._lib.lib(), mf._lib
    name = export.split(":")[0]

    def call(**kw):
        return _pair_adagrad(lib, **kw) if name == "mf_update_pair_adagrad" else _pair(lib, int(export.endswith("adam")), **kw)

    _refused(lib, call(d=48, n_rows_a=BIG), L.MF_EINVAL, name, "width")                              # the width before the table's size
    _refused(lib, call(n_rows_a=BIG, n_a=70000), L.MF_ENOTSUP, name, "too large")                    # the table's size before the lengths
    _refused(lib, call(n_a=0, short_b=1), L.MF_ENOTSUP, name, "list lengths")                        # the lengths before the workspace
