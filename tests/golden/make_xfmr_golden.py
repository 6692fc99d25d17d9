#!/usr/bin/env python3
"""Generate ``tests/golden/xfmr_h32_l1_a4_i32_L16.npz``: what ``transformers.models.bert.BertModel`` in eval mode (CPU,
fp32) computes for the sequence form of the tower -- ``BertModel(inputs_embeds=..., attention_mask=...)``, then mean / max /
cls pooling over the valid positions and L2-normalisation -- and, for the scalar ``sum(u . c)`` of the mean-pooled
outputs, its gradients with respect to ``inputs_embeds`` and every weight.  Data only: the GPU tests read the fixture and
the spec of ``tests/test_xfmr_tower_cpu.py``, never transformers.

    python tests/golden/make_xfmr_golden.py

Keys: ``cfg.*`` (h, layers, heads, inter, L, B), ``w.<state_dict name>``, ``inputs_embeds`` [B, L, h] (zero rows = padding),
``mask`` [B, L], ``c`` [B, h], ``u.mean`` / ``u.max`` / ``u.cls`` [B, h] (0 for an empty list), ``d_inputs_embeds``,
``dw.<state_dict name>``.
"""
from __future__ import annotations

import pathlib

import numpy as np
import torch
import torch.nn.functional as F
from transformers.models.bert import BertConfig, BertModel

H, LAYERS, HEADS, INTER, L, B = 32, 1, 4, 32, 16, 8
LENGTHS = [0, 1, 9, 16, 5, 16, 2, 12]


def pooled(hidden, mask, mode):
    out = []
    for b in range(hidden.shape[0]):
        n = int(mask[b].sum())
        if n == 0:
            out.append(torch.zeros(hidden.shape[2]))
            continue
        y = hidden[b, :n]
        p = y.mean(0) if mode == "mean" else y.max(0).values if mode == "max" else y[0]
        out.append(F.normalize(p, dim=0, eps=1e-12))
    return torch.stack(out)


def main() -> None:
    torch.manual_seed(20261016)
    model = BertModel(BertConfig(vocab_size=4, hidden_size=H, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                                 intermediate_size=INTER, hidden_act="gelu", max_position_embeddings=L), add_pooling_layer=False).eval()
    with torch.no_grad():                       # away from the initialiser's near-zero weights and unit LayerNorms
        for p in model.parameters():
            p.add_(torch.randn_like(p) * 0.15)
    params = {k: p for k, p in model.named_parameters() if "word_embeddings" not in k}
    mask = torch.zeros(B, L, dtype=torch.int64)
    for b, n in enumerate(LENGTHS):
        mask[b, :n] = 1
    x = F.normalize(torch.randn(B, L, H), dim=2) * mask[:, :, None]
    x.requires_grad_(True)
    c = torch.randn(B, H)
    hidden = model(inputs_embeds=x, attention_mask=mask).last_hidden_state
    out = {f"cfg.{k}": np.int64(v) for k, v in (("h", H), ("layers", LAYERS), ("heads", HEADS), ("inter", INTER), ("L", L), ("B", B))}
    out.update({f"w.{k}": p.detach().numpy().copy() for k, p in params.items()})
    out.update(inputs_embeds=x.detach().numpy().copy(), mask=mask.numpy(), c=c.numpy())
    for mode in ("mean", "max", "cls"):
        out[f"u.{mode}"] = pooled(hidden, mask, mode).detach().numpy().copy()
    (pooled(hidden, mask, "mean") * c).sum().backward()
    out["d_inputs_embeds"] = x.grad.numpy().copy()
    for k, p in params.items():
        out[f"dw.{k}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    path = pathlib.Path(__file__).resolve().parent / f"xfmr_h{H}_l{LAYERS}_a{HEADS}_i{INTER}_L{L}.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
