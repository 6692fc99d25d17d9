#!/usr/bin/env python3
"""SHA-256 of every tensor the transformer user tower produces on a set of small seeded worlds: what two builds of the library
must agree on bit for bit when a change is meant to leave the arithmetic alone.

    python tools/xfmr_bits.py --out profiles/xfmr_bits.json
    MF_HIP_LIB=path/to/parent/libmf_hip.so python tools/xfmr_bits.py --label parent --out parent.json    # then compare "digests"

Worlds: h in {32, 64, 128} (4 heads, I = 96 / 64 / 256), one and two layers, 300 table rows, B = 37 users with ragged lists of 0 to
99 entries (padding zeros, negative and too-large ids among them), L = 64.  Per world: the three pooling modes x both normalise
flags on and off x dropout off and 0.1 / 0.1 (seed 7) x fp32 and bf16-mixed.  Per configuration one training forward, one
backward, the coalesce and one SGD step on the table (``optim.SparseSGD``): a digest of ``u``, of each of the 4 + 16 per layer
dense gradients and of the table after the step; at fp32 without dropout also of ``encode(path="fused")``.  The file holds one
digest per configuration -- the SHA-256 of its tensors' names and digests, in that order -- so that it stays small enough to
keep; ``--tensors`` adds the 4,356 digests themselves, which is how a differing configuration is narrowed down to a tensor.
Every input comes from CPU generators, so the digests depend on the library alone.  Not imported by the package; no test
runs it.
"""
from __future__ import annotations

import argparse
import hashlib
import importlib
import itertools
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
DEV = "cuda:0"
ROWS, USERS, L = 300, 37, 64
WORLDS = [(h, layers) for h in (32, 64, 128) for layers in (1, 2)]
INTER = {32: 96, 64: 64, 128: 256}


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def combined(tensors: dict) -> str:
    return hashlib.sha256("\n".join(f"{k} {v}" for k, v in tensors.items()).encode()).hexdigest()


def lists(rng) -> list:
    out = []
    for n in rng.integers(0, 100, USERS).tolist():
        lst = rng.integers(1, ROWS, n)
        bad = rng.random(n) < 0.15                             # noqa: PLR2004
        lst[bad] = rng.choice([0, -3, ROWS, ROWS + 9], int(bad.sum()))
        out.append(lst.tolist())
    out[5] = []
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "xfmr_bits.json"))
    ap.add_argument("--tensors", action="store_true", help="also write every tensor's digest")
    ap.add_argument("--label", help="what to call the library in the output (default: its path)")
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    res = {"library": args.label or str(mf._lib.LIB_PATH), "digests": {}}
    tensors = {}
    for h, layers in WORLDS:
        g = torch.Generator().manual_seed(1000 * h + layers)
        rng = np.random.default_rng(h + layers)
        table = torch.randn(ROWS, h, generator=g) / h ** 0.5
        ll = lists(rng)
        off = torch.tensor(np.cumsum([0] + [len(x) for x in ll]), dtype=torch.int64, device=DEV)
        hist = (off[:-1], off[1:], torch.tensor([i for x in ll for i in x], dtype=torch.int64, device=DEV))
        c = torch.randn(USERS, h, generator=g).to(DEV)
        item0 = mf.models.EmbeddingTower(ROWS, h, device=DEV)
        probe = mf.models.HistoryTransformerTower(item0, num_hidden_layers=layers, intermediate_size=INTER[h], max_history=L)
        params = [(1.0 if p.ndim == 1 and k % 2 == 0 else 0.0) + 0.2 * torch.randn(p.shape, generator=g)   # (LayerNorm weights: about 1)
                  for k, p in enumerate(probe.encoder_parameters())]
        for mode, (n_i, n_u), p_drop, prec in itertools.product(("mean", "max", "cls"), ((True, True), (False, False)), (0.0, 0.1),
                                                                ("fp32", "bf16-mixed")):
            item = mf.models.EmbeddingTower(ROWS, h, normalize=n_i, device=DEV)
            user = mf.models.HistoryTransformerTower(item, num_hidden_layers=layers, num_attention_heads=4, intermediate_size=INTER[h],
                                                     pooling_mode=mode, max_history=L, normalize=n_u, hidden_dropout_prob=p_drop,
                                                     attention_probs_dropout_prob=p_drop, dropout_seed=7, precision=prec)
            with torch.no_grad():
                item.weight.copy_(table)
                for p, v in zip(user.encoder_parameters(), params):
                    p.copy_(v)
            user.train()
            name = f"h{h}-l{layers}-{mode}-ni{int(n_i)}-nu{int(n_u)}-p{p_drop}-{prec}"
            u = user(hist)
            (u * c).sum().backward()
            out = {"u": digest(u)}
            for k, p in enumerate(user.encoder_parameters()):
                out[f"grad{k}"] = digest(p.grad)
            mf.optim.SparseSGD([item.weight], lr=0.5).step()
            out["table"] = digest(item.weight)
            if p_drop == 0.0 and prec == "fp32":
                out["encode_fused"] = digest(user.encode(hist, path="fused"))
            tensors[name], res["digests"][name] = out, combined(out)
    torch.cuda.synchronize()
    res["configurations"], res["tensors"] = len(tensors), sum(len(v) for v in tensors.values())
    res["all"] = combined(res["digests"])
    if args.tensors:
        res["tensor_digests"] = tensors
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1))
    print(f"{res['configurations']} configurations, {res['tensors']} tensors, all = {res['all']}; wrote {out}")


if __name__ == "__main__":
    main()
