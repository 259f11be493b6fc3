"""numpy restatement of the FLDetector kernels (include/plato_agg.h, "FLDetector") and of a round of
``AggregationRound.launch_fldetector``: bit-defined everywhere except the order of the float64 sums of the
dots and the squared distances, which are ``math.fsum`` here (the correctly rounded exact sum) and a fixed
chunked order on the device, within D * 2^-53 * sum|terms| of it.

The scalars of the host (the 2N x 2N solve, the normalisation, the history mean and the 2-means split)
are ``plato_amd.detectors``' own functions, held to the reference by tests/test_fldetector.py.
"""

from __future__ import annotations

import math

import numpy as np

from plato_amd import detectors as host

F32, F64 = np.float32, np.float64


def columns(xf: np.ndarray, xi: np.ndarray) -> np.ndarray:
    """[K, D] float32: the rows as flat rows, counters promoted (round to nearest even)."""
    return np.concatenate([xf.astype(F32), xi.astype(F32)], axis=1)


def flat(bf: np.ndarray, bi: np.ndarray) -> np.ndarray:
    return np.concatenate([bf.astype(F32), bi.astype(F32)])


def deltas(xf, xi, bf, bi) -> np.ndarray:
    """[K, D] float32: the fp32 difference, and the wrapping int64 difference rounded once."""
    with np.errstate(over="ignore", invalid="ignore"):
        df = (xf - bf[None, :]).astype(F32)
        di = (xi.astype(np.uint64) - bi.astype(np.uint64)[None, :]).astype(np.int64)
    return np.concatenate([df, di.astype(F32)], axis=1)


def detect_means(xf, xi, bf, bi, last_w, last_g):
    """(g, v, s_new, y_new, b_flat) of plato_agg_detect_means: float64 sums over k in table order."""
    k = xf.shape[0]
    d, c, b = deltas(xf, xi, bf, bi), columns(xf, xi), flat(bf, bi)
    with np.errstate(over="ignore", invalid="ignore"):
        sd, sv = np.zeros(b.size, dtype=F64), np.zeros(b.size, dtype=F64)
        for r in range(k):
            sd = sd + d[r].astype(F64)
            sv = sv + (c[r] - last_w).astype(F32).astype(F64)
        g = (sd / F64(k)).astype(F32)
        v = (sv / F64(k)).astype(F32)
        return g, v, (b - last_w).astype(F32), (g - last_g).astype(F32), b


def dot(a: np.ndarray, b: np.ndarray):
    """(math.fsum of the float64 products, sum of their magnitudes)."""
    with np.errstate(over="ignore", invalid="ignore"):
        terms = a.astype(F64) * b.astype(F64)
    if not np.all(np.isfinite(terms)):
        return float(np.sum(terms)), float("inf")  # IEEE propagation: nan, or an infinity of one sign
    return math.fsum(terms), math.fsum(np.abs(terms))


def rows_dots(rows, vecs):
    """([R, m] dots, [R, m] sums of |terms|)."""
    out = np.array([[dot(r, v) for v in vecs] for r in rows], dtype=F64).reshape(len(rows), len(vecs), 2)
    return out[:, :, 0], out[:, :, 1]


def predict(rows, a, sigma, last_g, v) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        acc = np.zeros(v.size, dtype=F64)
        for j, row in enumerate(rows):
            acc = acc + F64(a[j]) * row.astype(F64)
        t = last_g.astype(F64) + F64(sigma) * v.astype(F64)
        return (t - acc).astype(F32)


def sqdist(pred, d):
    """([K] squared distances, [K] sums of the terms' magnitudes)."""
    out, mag = [], []
    for row in d:
        with np.errstate(over="ignore", invalid="ignore"):
            t = pred.astype(F64) - row.astype(F64)
            terms = t * t
        if not np.all(np.isfinite(terms)):
            out.append(float(np.sum(terms)))
            mag.append(float("inf"))
        else:
            out.append(math.fsum(terms))
            mag.append(out[-1])
    return np.array(out, dtype=F64), np.array(mag, dtype=F64)


def bound(d: int, magnitude):
    """The reduction's distance from the exact sum: D * 2^-53 * sum|terms| (plato_agg_trust_stats (c))."""
    return d * 2.0 ** -53 * np.asarray(magnitude, dtype=F64)


class Record:
    """The detector's state as ``plato_amd.detectors.FLDetectorState`` keeps it, in numpy on the host."""

    def __init__(self, dim: int):
        self.dim = dim
        self.s, self.y = [], []
        self.last_w, self.last_g = np.zeros(dim, dtype=F32), np.zeros(dim, dtype=F32)
        self.history: dict = {}
        self.sy, self.ss, self.yy = np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0)

    @classmethod
    def from_reference(cls, s_rows, y_rows, last_w, last_g, scores, index):
        """From the reference's record (flat vectors in state-dict order; ``index`` = arena_index)."""
        def arena(v):
            out = np.empty(index.size, dtype=F32)
            out[index] = np.asarray(v, dtype=F32)
            return out

        rec = cls(index.size)
        rec.s, rec.y = [arena(r) for r in s_rows], [arena(r) for r in y_rows]
        rec.last_w, rec.last_g = arena(last_w), arena(last_g)
        rec.history = {k: list(v) for k, v in scores.items()}
        rec.sy, rec.ss, rec.yy = rec.full_gram()
        return rec

    def full_gram(self):
        n = len(self.s)
        g = rows_dots(self.s + self.y, self.s + self.y)[0] if n else np.zeros((0, 0))
        return g[:n, n:].copy(), g[:n, :n].copy(), np.diag(g[n:, n:]).copy()

    def round(self, xf, xi, bf, bi, ids) -> dict:
        n, k = len(self.s), xf.shape[0]
        g, v, s_new, y_new, b = detect_means(xf, xi, bf, bi, self.last_w, self.last_g)
        dots = rows_dots(self.s + self.y + [s_new, y_new], [v, s_new, y_new])[0]
        info = {"distances": None, "scores": None, "malicious": [], "g": g, "v": v, "s_new": s_new, "y_new": y_new,
                "dots": dots}
        now = [None] * k
        if n:
            coef = host.lbfgs_coefficients(self.sy, self.ss, self.yy[n - 1], dots[:n, 0], dots[n:2 * n, 0])
            pred = predict(self.s + self.y, coef["a"], coef["sigma"], self.last_g, v)
            d2 = sqdist(pred, deltas(xf, xi, bf, bi))[0]
            now = list(host.normalised_distances(d2))
            scores = np.array([host.history_score(self.history.get(c, ()), d) for c, d in zip(ids, now)], dtype=F32)
            info.update(distances=np.array(now, dtype=F32), scores=scores, malicious=host.two_means_1d(scores)[0],
                        d2=d2, pred=pred, sigma=coef["sigma"], cond=coef["cond"], a=coef["a"])
        for c, d in zip(ids, now):
            self.history.setdefault(c, []).append(d)
        sy, ss = np.zeros((n + 1, n + 1)), np.zeros((n + 1, n + 1))
        sy[:n, :n], ss[:n, :n] = self.sy, self.ss
        sy[n, :n], sy[:n, n], sy[n, n] = dots[n:2 * n, 1], dots[:n, 2], dots[2 * n, 2]
        ss[n, :n] = ss[:n, n] = dots[:n, 1]
        ss[n, n] = dots[2 * n, 1]
        self.sy, self.ss, self.yy = sy, ss, np.append(self.yy, dots[2 * n + 1, 2])
        self.s.append(s_new)
        self.y.append(y_new)
        self.last_w, self.last_g = b, g
        return info
