"""Fl-trust's scalars on the host: torch CPU fp32 ops over the float64 reductions of the device.

Restates the scalar part of ``aggregations.fl_trust`` (the reference's examples/detector/aggregations.py:
403-453) on the ``3K + 1`` float64 sums that ``plato_agg_trust_stats`` computes in one pass over the
staged rows, where the reference calls ``torch.dot`` and ``torch.norm`` per client:

    cos_k = dot(x_k, m) / (|m| + 1e-9) / (|x_k| + 1e-9)          aggregations.py:414-418
    c     = torch.maximum(cos, torch.tensor(0))                   :426
    w     = c / (torch.sum(c) + 1e-9)                             :427
    out   = sum_k x_k * w_k / |x_k + 1e-9| * |m|                  :429-441 (plato_agg_scaled_sum)

The norms are ``fp32(sqrt(float64 sum))`` and the dots ``fp32(float64 sum)``: one rounding each, where
the reference's fp32 BLAS dot and ATen norm carry an error that grows with the model size.  The square
root is taken in float64, so a squared norm above the fp32 maximum still gives a finite norm where the
reference gives inf.  Everything after that is the reference's own expression on fp32 tensors and Python
floats, evaluated by the same torch CPU ops (elementwise over the clients where the reference loops over
0-dim tensors: the same IEEE operations per element): given the same fp32 dots and norms the normalised
weights are the reference's bit for bit.  A NaN cosine makes ``torch.sum`` NaN and with it every weight,
as in the reference; K = 1 needs no special case.
"""

from __future__ import annotations

import numpy as np
import torch

EPS = 1e-9  # the reference's literal


def weights_from_scalars(dots, norms, nm, eps: float = EPS):
    """(cos, weights) as float32 arrays from the fp32 dots [K], norms [K] and the mean's norm, by the
    reference's expressions (aggregations.py:414-427)."""
    dots = torch.from_numpy(np.ascontiguousarray(dots, dtype=np.float32))
    norms = torch.from_numpy(np.ascontiguousarray(norms, dtype=np.float32))
    norm_re = torch.tensor(float(np.float32(nm)), dtype=torch.float32)
    # one elementwise expression for the reference's loop over the clients: the same IEEE fp32 additions
    # and divisions per element (tests/test_fltrust.py holds it to the reference's bits)
    cos_sims = dots / (norm_re + eps) / (norms + eps)
    cos = cos_sims.clone()
    cos_sims = torch.maximum(cos_sims, torch.tensor(0))
    normalized = cos_sims / (torch.sum(cos_sims) + eps)
    return cos.numpy(), normalized.numpy()


def fltrust_weights(stats, k: int, eps: float = EPS) -> dict:
    """Fl-trust's scalars from the ``3k + 1`` doubles of ``plato_agg_trust_stats``, all float32:

    ``nm`` |m|; ``dots`` [k] dot(x_k, m); ``norms`` [k] |x_k|; ``norms_eps`` [k] |x_k + eps|; ``cos`` [k]
    the cosines before the clip; ``weights`` [k] the normalised clipped cosines; ``div`` [k] the divisor
    of each row in ``plato_agg_scaled_sum`` (``norms_eps``).  ``plato_agg_scaled_sum(mul=weights,
    div=div, post=nm)`` is the aggregate.
    """
    k = int(k)
    stats = np.asarray(stats, dtype=np.float64).reshape(-1)
    if k < 1 or stats.size != 3 * k + 1:
        raise ValueError(f"Fl-trust statistics of {k} clients are {3 * max(k, 0) + 1} doubles, got {stats.size}")
    with np.errstate(invalid="ignore", over="ignore"):  # NaN stays NaN; a dot beyond fp32 is +-inf, as fp32 says
        dots = stats[:k].astype(np.float32)
        norms = np.sqrt(stats[k:2 * k]).astype(np.float32)
        norms_eps = np.sqrt(stats[2 * k:3 * k]).astype(np.float32)
        nm = np.float32(np.sqrt(stats[3 * k]))
    cos, weights = weights_from_scalars(dots, norms, nm, eps)
    return {"nm": nm, "dots": dots, "norms": norms, "norms_eps": norms_eps, "cos": cos, "weights": weights,
            "div": norms_eps.copy()}
