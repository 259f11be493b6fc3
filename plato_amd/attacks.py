"""Host side of the attack simulation of the reference's detector example (examples/detector/attacks.py):
the scalars of ``LIE`` and the lambda searches of ``Min-Max`` and ``Min-Sum``.  The vectors are formed on
the device (``RobustLaunches.launch_attack``); what is here is O(A) float64 work per search step.

The searches restate the reference's loop in what concerns lambda: an fp32 ``lambda_value`` that starts at
10000 and moves by fp32 halving steps until ``|lambda_succ - lambda_value| <= 1e-5``.  Only the predicate is
evaluated differently.  With ``u`` a delta row, the reference forms ``|u - (avg - lam * p)|^2`` in fp32 with
one pass over the rows per step; here it is expanded into dots and squared norms of ``u``, ``avg`` and the
actual fp32 vector ``p``, which ``plato_agg_trust_stats`` yields in float64 once::

    |u - avg + lam p|^2 = |u|^2 + |avg|^2 + lam^2 |p|^2 - 2 u.avg + 2 lam u.p - 2 lam avg.p

The expansion cancels when the rows are nearly equal: its error is within D * 2^-53 of the sum of the
magnitudes of its terms, far below the fp32 error of the reference's own sum unless the rows
agree to about three digits.  Rows that are exactly equal are handled apart: the threshold is then exactly 0
and no lambda > 0 can meet it.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

#: ``clients.attack_type`` -> the kind of ``launch_attack``; every other attack stays on the host
KINDS = {"LIE": "lie", "Lambda_attack": "lambda", "Min-Max": "minmax", "Min-Sum": "minsum"}
LAMBDA_INIT = np.float32(10000.0)
LAMBDA_STOP = 1e-5
MIN_SUM_INIT = 5e10  # the reference's initial min_sum_distance


# The Cephes rational approximations of erf (|x| < 1) and erfc (1 <= x < 8) that scipy.special.ndtr
# evaluates (netlib cephes/ndtr.c), so that z has scipy.stats.norm.cdf's float64 bits without scipy:
# math.erf, the platform's libm, differs from it in the last bit for about half of all arguments.
_ERF_T = (9.60497373987051638749E0, 9.00260197203842689217E1, 2.23200534594684319226E3,
          7.00332514112805075473E3, 5.55923013010394962768E4)
_ERF_U = (3.35617141647503099647E1, 5.21357949780152679795E2, 4.59432382970980127987E3,
          2.26290000613890934246E4, 4.92673942608635921086E4)
_ERFC_P = (2.46196981473530512524E-10, 5.64189564831068821977E-1, 7.46321056442269912687E0,
           4.86371970985681366614E1, 1.96520832956077098242E2, 5.26445194995477358631E2,
           9.34528527171957607540E2, 1.02755188689515710272E3, 5.57535335369399327526E2)
_ERFC_Q = (1.32281951154744992508E1, 8.67072140885989742329E1, 3.54937778887819891062E2,
           9.75708501743205489753E2, 1.82390916687909736289E3, 2.24633760818710981792E3,
           1.65666309194161350182E3, 5.57535340817727675546E2)


def _horner(x: float, coefs, monic: bool) -> float:
    acc = x + coefs[0] if monic else coefs[0]
    for c in coefs[1:]:
        acc = acc * x + c
    return acc


def normal_cdf(a: float) -> float:
    """The normal distribution function in float64, operation for operation as ``scipy.special.ndtr``."""
    x = a * math.sqrt(0.5)
    z = abs(x)
    if z < 1.0:
        return 0.5 + 0.5 * (x * _horner(x * x, _ERF_T, False) / _horner(x * x, _ERF_U, True))
    if z < 8.0:
        y = 0.5 * ((math.exp(-x * x) * _horner(z, _ERFC_P, False)) / _horner(z, _ERFC_Q, True))
    else:
        y = 0.5 * math.erfc(z)  # below 2^-53 of 1: the form no longer shows
    return 1.0 - y if x > 0 else y


def lie_z(per_round: int, num_attackers: int) -> float:
    """``norm.cdf((n - s) / n)`` with ``s = n / 2 + 1 - A`` (attacks.py:191-193), in float64."""
    n = per_round
    s = n / 2 + 1 - num_attackers
    return normal_cdf((n - s) / n)


def halving_search(meets, keep_failed: bool = False) -> np.float32:
    """The reference's search: ``meets(lam)`` says whether lambda (an fp32 value) keeps the poisoned
    update within the threshold.  ``keep_failed`` is Min-Sum's ``else`` branch, which also records the
    lambda that failed ("incase no succ"): its result is the last lambda tried."""
    two = np.float32(2.0)
    lam = step = LAMBDA_INIT
    succ = np.float32(0.0)
    while abs(np.float32(succ - lam)) > LAMBDA_STOP:
        if meets(lam):
            succ = lam
            lam = np.float32(lam + np.float32(step / two))
        else:
            if keep_failed:
                succ = lam
            lam = np.float32(lam - np.float32(step / two))
        step = np.float32(step / two)
    return succ


@dataclass
class SearchStats:
    """float64 dots and squared norms of the A delta rows ``u``, of ``avg`` and of the fp32 vector ``p``."""
    uu: np.ndarray  # [A] |u_k|^2
    ua: np.ndarray  # [A] u_k . avg
    up: np.ndarray  # [A] u_k . p
    aa: float       # |avg|^2
    pp: float       # |p|^2
    ap: float       # avg . p

    def sqdist(self, lam) -> np.ndarray:
        """[A] ``|u_k - avg + lam p|^2`` in float64."""
        lam = float(lam)
        with np.errstate(invalid="ignore", over="ignore"):
            return (self.uu + self.aa + lam * lam * self.pp - 2.0 * self.ua + 2.0 * lam * self.up
                    - 2.0 * lam * self.ap)


def min_max_threshold(dist: np.ndarray) -> float:
    """The largest squared distance between two delta rows (NaN if any is)."""
    return float(np.max(dist))


def min_sum_threshold(dist: np.ndarray) -> float:
    """The smallest row sum of the distance matrix, capped by the reference's 5e10.  The rows are summed
    in float64; the reference sums each in fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.minimum(MIN_SUM_INIT, np.min(dist.sum(axis=1))))


def _search(stats: SearchStats, threshold: float, reduce, keep_failed: bool) -> np.float32:
    if threshold == 0.0:  # identical rows: |lam p|^2 > 0 for every lambda > 0
        return halving_search(lambda lam: False, keep_failed)
    with np.errstate(invalid="ignore"):
        return halving_search(lambda lam: bool(reduce(stats.sqdist(lam)) <= threshold), keep_failed)


def min_max_lambda(stats: SearchStats, dist: np.ndarray) -> np.float32:
    """``Min-Max`` (attacks.py:262-284): the largest lambda the search finds whose poisoned update is no
    further from any delta row than the two furthest rows are from each other; 0 if none."""
    return _search(stats, min_max_threshold(dist), np.max, False)


def min_sum_lambda(stats: SearchStats, dist: np.ndarray) -> np.float32:
    """``Min-Sum`` (attacks.py:394-418): the sum of the squared distances against the smallest row sum."""
    return _search(stats, min_sum_threshold(dist), np.sum, True)
