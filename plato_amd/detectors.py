"""FLDetector (the reference's examples/detector/detectors.py: ``fl_detector``, ``lbfgs``) with its record on
the device.

Every round the reference keeps N global-weight differences S and N mean-update differences Y, predicts the
round's mean update from them by the L-BFGS compact form and scores each client by the distance of its
update to the prediction.  Here the record lives in HBM (:class:`FLDetectorState`) and everything that
streams the model is a kernel of ``csrc/detect.hip``; the host keeps what is small: the float64 Gram cache
of the record, the 2N x 2N solve, the K scores and their clustering::

    sigma = (s_last . y_last) / (y_last . y_last)                        detectors.py:80-84
    mat   = [[sigma * S S^T, L], [L^T, -diag(S Y^T)]], L = strict lower triangle of S Y^T     :76-89
    p     = [sigma * (S v); Y v]                                         :97-99
    c     = solve(mat, p)               (the reference: torch.inverse(mat) @ p in fp32)
    pred  = last_g + sigma * v - [sigma * S^T, Y^T] c                    :96-106, :359
    score = history mean of |pred - delta_k| / sum_k |pred - delta_k|   :362-376

Divergences from the reference, all documented in DESIGN.md §25: dots, means and distances are float64
sums on the device and the system is solved in float64; the square root is taken in float64; the
clustering is the exact optimal split (:func:`two_means_1d`) where the reference runs scikit-learn's
randomly initialised k-means; the record is not pickled to the working directory every round
(:meth:`FLDetectorState.state_dict` is the checkpoint).
"""

from __future__ import annotations

from typing import Mapping, Sequence

import numpy as np
import torch

from . import _lib

BLOCK_ROWS = 16  # record rows per device allocation; rows never move once written


# ------------------------------------------------------------------ host scalars
def two_means_1d(scores) -> tuple[list[int], list[int]]:
    """(malicious, clean) positions of the exact 2-means clustering of K scalars: the split of the sorted
    scores with the least within-cluster sum of squares, which is the global optimum of the objective
    the reference's ``KMeans(n_clusters=2)`` descends on (an optimal 1-D clustering is contiguous).  The
    cluster with the lower mean is clean, as in ``detection()``.  Both lists are ascending.

    Equal scores are never separated.  Two splits of equal cost: the one that flags fewer clients.  All
    scores equal (K = 1 included): one cluster, nobody is flagged (the reference's k-means then returns
    a single label and its ``detection()`` flags everybody; a documented divergence).  Non-finite
    scores raise ``ValueError``.
    """
    x = np.asarray(scores, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(x)):
        raise ValueError("FLDetector: non-finite malicious score")
    k = x.size
    order = np.argsort(x, kind="stable")
    xs = x[order]
    best, best_cost = None, np.inf
    for cut in range(k - 1, 0, -1):  # clean = the first `cut` sorted scores; larger clean clusters first
        if xs[cut - 1] == xs[cut]:
            continue
        lo, hi = xs[:cut], xs[cut:]
        cost = float(np.sum((lo - lo.mean()) ** 2) + np.sum((hi - hi.mean()) ** 2))
        if cost < best_cost:
            best, best_cost = cut, cost
    if best is None:
        return [], list(range(k))
    return sorted(int(i) for i in order[best:]), sorted(int(i) for i in order[:best])


def lbfgs_coefficients(sy: np.ndarray, ss: np.ndarray, yy_last: float, s_v: np.ndarray, y_v: np.ndarray) -> dict:
    """The scalars of ``lbfgs()`` from the float64 Gram matrices S Y^T (``sy``) and S S^T (``ss``), y_last .
    y_last and the dots S v, Y v: ``sigma``, the 2N coefficients ``a`` = [sigma * c[:N], c[N:]] of
    ``plato_agg_lbfgs_predict`` over the rows [S; Y], and ``cond``, the 2-norm condition number of the
    system.  A singular or non-finite system raises ``ValueError`` (the reference raises from
    ``torch.inverse``)."""
    sy = np.asarray(sy, dtype=np.float64)
    ss = np.asarray(ss, dtype=np.float64)
    n = sy.shape[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sigma = np.float64(sy[n - 1, n - 1]) / np.float64(yy_last)
        low = np.tril(sy, -1)
        mat = np.block([[sigma * ss, low], [low.T, -np.diag(np.diag(sy))]])
        p = np.concatenate([sigma * np.asarray(s_v, dtype=np.float64), np.asarray(y_v, dtype=np.float64)])
    if not (np.isfinite(sigma) and np.all(np.isfinite(mat)) and np.all(np.isfinite(p))):
        raise ValueError("FLDetector: the L-BFGS system is not finite (y_last = 0 after two identical rounds?)")
    try:
        c = np.linalg.solve(mat, p)
        cond = float(np.linalg.cond(mat))
    except np.linalg.LinAlgError as exc:
        raise ValueError(f"FLDetector: the L-BFGS system is singular ({exc})") from None
    if not (np.all(np.isfinite(c)) and np.isfinite(cond)):
        raise ValueError("FLDetector: the L-BFGS system is singular")
    return {"sigma": float(sigma), "a": np.concatenate([sigma * c[:n], c[n:]]), "cond": cond, "mat": mat, "p": p}


def normalised_distances(d2) -> np.ndarray:
    """float32 [K]: ``sqrt(d2)`` in float64, divided by its float64 sum, rounded once (the reference:
    an fp32 norm divided by its fp32 ``np.sum``).  A non-finite or all-zero set raises ``ValueError``."""
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.sqrt(np.asarray(d2, dtype=np.float64))
        total = float(np.sum(dist))
    if not np.all(np.isfinite(dist)) or not np.isfinite(total) or total == 0.0:
        raise ValueError("FLDetector: non-finite or all-zero distances to the prediction")
    return (dist / total).astype(np.float32)


def history_score(past: Sequence, now: np.float32) -> np.float32:
    """``sum(scores) / len(scores)`` of detectors.py:373-376 over a client's earlier distances (``None``
    entries skipped) and this round's: the sequential fp32 sum, one fp32 division."""
    vals = [np.float32(v) for v in past if v is not None] + [np.float32(now)]
    acc = vals[0]
    for v in vals[1:]:
        acc = np.float32(acc + v)
    return np.float32(acc / np.float32(len(vals)))


def arena_index(layout) -> np.ndarray:
    """For a flat vector in state-dict order (the reference's ``flatten_weight``): the position of every
    element in a flat row, [fp32 region | int64 region]."""
    if not layout.packed:
        raise ValueError("FLDetector sums over the whole fp32 region: the arena must have no alignment padding")
    parts = [np.arange(e.numel, dtype=np.int64) + (e.offset if e.region == "f32" else layout.n_f32 + e.offset)
             for e in layout.entries]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def _flat_host(vec, index: np.ndarray) -> torch.Tensor:
    """A reference flat vector (state-dict order) as a float32 host tensor in arena order."""
    src = torch.as_tensor(vec).detach().to(torch.float32).reshape(-1).cpu()
    if src.numel() != index.size:
        raise ValueError(f"FLDetector record vector has {src.numel()} elements, the model {index.size}")
    out = torch.empty(index.size, dtype=torch.float32)
    out[torch.from_numpy(index)] = src
    return out


# ------------------------------------------------------------------ the record
class FLDetectorState:
    """The detector's record, kept across rounds: the S and Y rows in HBM (allocated ``BLOCK_ROWS`` at a
    time and reached through a pointer table: a grown record copies nothing), ``last_w`` and ``last_g``,
    every client's distance history and the float64 Gram cache (S Y^T whole, S S^T, the diagonal of
    Y Y^T), which each round extends by one row and column from its one ``plato_agg_rows_dots`` pass.

    ``max_records=None`` lets the record grow without bound, as the reference's does (``window_size = 0``,
    never trimmed); an integer keeps the newest rows only (a divergence).  A state filled by
    :meth:`load_state_dict` or :meth:`load_reference_record` holds host tensors until its first round
    moves them to the round's device; a Gram cache that was not loaded is recomputed there.
    """

    def __init__(self, max_records: int | None = None):
        if max_records is not None and int(max_records) < 1:
            raise ValueError("max_records must be None or at least 1")
        self.max_records = None if max_records is None else int(max_records)
        self.reset()

    def reset(self) -> None:
        self.signature = None
        self.device = None
        self.dim = 0
        self.s_rows: list[torch.Tensor] = []   # flat rows, oldest first (host tensors while detached)
        self.y_rows: list[torch.Tensor] = []
        self.last_w: torch.Tensor | None = None
        self.last_g: torch.Tensor | None = None
        self.history: dict = {}                 # client id -> [np.float32 | None]
        self.sy = np.zeros((0, 0))
        self.ss = np.zeros((0, 0))
        self.yy = np.zeros(0)
        self._cache_ok = True
        self._free: list[torch.Tensor] = []     # unused rows of the allocated blocks
        self._spare: list[torch.Tensor] = []    # the buffers last_w / last_g alternate with
        self.rounds = 0

    def __len__(self) -> int:
        return len(self.s_rows)

    # -------------------------------------------------------------- checkpoints
    def state_dict(self) -> dict:
        """Host copies of everything the next round reads (blocks until the device has written them)."""
        host = lambda t: None if t is None else t.detach().cpu().clone()  # noqa: E731
        stack = lambda rows: (torch.stack([host(r) for r in rows]) if rows  # noqa: E731
                              else torch.zeros((0, self.dim), dtype=torch.float32))
        return {"signature": self.signature, "dim": self.dim, "max_records": self.max_records, "rounds": self.rounds,
                "S": stack(self.s_rows), "Y": stack(self.y_rows), "last_w": host(self.last_w),
                "last_g": host(self.last_g), "history": {k: list(v) for k, v in self.history.items()},
                "gram": {"sy": self.sy.copy(), "ss": self.ss.copy(), "yy": self.yy.copy()} if self._cache_ok else None}

    def load_state_dict(self, state: Mapping) -> None:
        s, y = state["S"], state["Y"]
        if s.shape != y.shape or s.dim() != 2 or s.shape[1] != state["dim"]:
            raise ValueError("FLDetector state: S and Y must be [N, D] with the same N")
        self.reset()
        self.signature, self.dim = state["signature"], int(state["dim"])
        self.max_records, self.rounds = state["max_records"], int(state["rounds"])
        self.s_rows = [r.to(torch.float32).clone() for r in s]
        self.y_rows = [r.to(torch.float32).clone() for r in y]
        self.last_w = None if state["last_w"] is None else state["last_w"].to(torch.float32).clone()
        self.last_g = None if state["last_g"] is None else state["last_g"].to(torch.float32).clone()
        self.history = {k: list(v) for k, v in state["history"].items()}
        gram = state.get("gram")
        if gram is None:
            self._cache_ok = len(self.s_rows) == 0
        else:
            self.sy, self.ss, self.yy = (np.array(gram[k], dtype=np.float64) for k in ("sy", "ss", "yy"))

    def load_reference_record(self, global_weights_record, gradients_record, last_weights, last_gradients,
                              malicious_score_dict, layout) -> None:
        """Take over the reference's record: the five objects it pickles to ``./record<pid>.pkl``, whose flat
        vectors are in state-dict order; ``layout`` (the model's ``ArenaLayout``) gives the arena order the
        rows are kept in.  The Gram cache is rebuilt on the device by the first round."""
        if len(global_weights_record) != len(gradients_record):
            raise ValueError("FLDetector record: as many global-weight rows as gradient rows")
        index = arena_index(layout)
        max_records = self.max_records
        self.reset()
        self.max_records = max_records
        self.signature, self.dim = layout.signature, int(index.size)
        self.s_rows = [_flat_host(r, index) for r in global_weights_record]
        self.y_rows = [_flat_host(r, index) for r in gradients_record]
        self.last_w, self.last_g = _flat_host(last_weights, index), _flat_host(last_gradients, index)
        self.history = {k: [None if v is None else np.float32(v) for v in vals]
                        for k, vals in malicious_score_dict.items()}
        self.rounds = len(self.s_rows)
        self._cache_ok = len(self.s_rows) == 0
        self._trim()

    # -------------------------------------------------------------- device residency
    def _take_row(self) -> torch.Tensor:
        if not self._free:
            block = torch.empty((BLOCK_ROWS, max(self.dim, 1)), dtype=torch.float32, device=self.device)
            self._free = [block[r, : self.dim] for r in range(BLOCK_ROWS - 1, -1, -1)]
        return self._free.pop()

    def _attach(self, layout, device) -> None:
        """Bind to ``layout`` and move host-held rows to ``device`` (first round, or after a load)."""
        dim = layout.n_f32 + layout.n_i64
        if self.signature is None:
            self.signature, self.dim = layout.signature, dim
        elif self.signature != layout.signature or self.dim != dim:
            raise ValueError("FLDetector: the round's model is not the one the record was kept for")
        if self.device is not None and self.device != device:
            raise ValueError(f"FLDetector: the record lives on {self.device}, the round on {device}")
        if self.device is None:
            self.device = device

            def up(t):
                row = self._take_row()
                row.copy_(t)
                return row

            self.s_rows = [up(r) for r in self.s_rows]
            self.y_rows = [up(r) for r in self.y_rows]
            zeros = lambda: torch.zeros(self.dim, dtype=torch.float32, device=device)  # noqa: E731
            self.last_w = zeros() if self.last_w is None else self.last_w.to(device)
            self.last_g = zeros() if self.last_g is None else self.last_g.to(device)
            self._spare = [torch.empty(self.dim, dtype=torch.float32, device=device) for _ in range(2)]

    def _table(self, extra: Sequence[torch.Tensor] = ()) -> torch.Tensor:
        """Device table of the row pointers [S_0 .. S_{N-1}, Y_0 .. Y_{N-1}, *extra]."""
        ptrs = [r.data_ptr() for r in (*self.s_rows, *self.y_rows, *extra)]
        return torch.from_numpy(np.asarray(ptrs, dtype=np.int64)).to(self.device)

    def rows_dots(self, rows: torch.Tensor, n_rows: int, vecs: Sequence[torch.Tensor], stream) -> np.ndarray:
        """[n_rows, m] float64 on the host: ``plato_agg_rows_dots`` of a device pointer table against m flat
        vectors.  Blocks."""
        m = len(vecs)
        nbytes = _lib.lib().plato_agg_rows_dots_workspace(n_rows, m, self.dim)
        work = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        out = torch.zeros((n_rows, m), dtype=torch.float64, device=self.device)  # nothing is written for D = 0
        vt = torch.from_numpy(np.asarray([v.data_ptr() for v in vecs], dtype=np.int64)).to(self.device)
        _lib.call("plato_agg_rows_dots", rows.data_ptr(), n_rows, vt.data_ptr(), m, self.dim, work.data_ptr(),
                  out.data_ptr(), stream.cuda_stream)
        return out.cpu().numpy()  # stream-ordered, blocking: work and vt are done with

    def full_gram(self, stream) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(S Y^T, S S^T, diag(Y Y^T)) recomputed from the rows: 2N rows against themselves, four vectors a
        call.  The cache holds the same bits (a dot's value depends on its two rows and D alone)."""
        n = len(self)
        if n == 0:
            return np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0)
        rows = [*self.s_rows, *self.y_rows]
        table = self._table()
        gram = np.concatenate([self.rows_dots(table, 2 * n, rows[j:j + 4], stream) for j in range(0, 2 * n, 4)], axis=1)
        return gram[:n, n:].copy(), gram[:n, :n].copy(), np.diag(gram[n:, n:]).copy()

    def _trim(self) -> None:
        if self.max_records is None:
            return
        while len(self.s_rows) > self.max_records:
            for rows in (self.s_rows, self.y_rows):
                row = rows.pop(0)
                if self.device is not None:
                    self._free.append(row)
            if self._cache_ok:
                self.sy, self.ss, self.yy = self.sy[1:, 1:], self.ss[1:, 1:], self.yy[1:]

    # -------------------------------------------------------------- one round
    def round(self, rnd, tf, ti, k: int, received_ids: Sequence, stream) -> dict:
        """One ``fl_detector`` call over the k staged rows of ``rnd`` (pointer tables ``tf``, ``ti``) and its
        baseline; returns what ``rnd.detector`` holds.  The record is extended only if nothing raised."""
        lay = rnd.layout
        self._attach(lay, rnd.engine.device)
        n_f, n_i, h = lay.n_f32, lay.n_i64, stream.cuda_stream
        base = rnd._base
        base_args = (base.f32.data_ptr() if n_f else None, base.i64.data_ptr() if n_i else None)
        if not self._cache_ok:  # a loaded record: its Gram matrices, once
            with rnd._timed("detector_gram", stream):
                self.sy, self.ss, self.yy = self.full_gram(stream)
            self._cache_ok = True
        n = len(self)
        g, w_next = self._spare
        v = torch.empty(self.dim, dtype=torch.float32, device=self.device)
        s_new, y_new = self._take_row(), self._take_row()
        try:
            with rnd._timed("detect_means", stream):
                _lib.call("plato_agg_detect_means", *rnd._regions(tf, ti), k, *base_args, self.last_w.data_ptr(),
                          self.last_g.data_ptr(), g.data_ptr(), v.data_ptr(), s_new.data_ptr(), y_new.data_ptr(),
                          w_next.data_ptr(), n_f, n_i, h)
            with rnd._timed("rows_dots", stream):
                dots = self.rows_dots(self._table((s_new, y_new)), 2 * n + 2, (v, s_new, y_new), stream)
            info = {"distances": None, "scores": None, "malicious": [], "sigma": None, "cond": None, "pred": None,
                    "records": n}
            now = [None] * k
            if n:
                coef = lbfgs_coefficients(self.sy, self.ss, self.yy[n - 1], dots[:n, 0], dots[n:2 * n, 0])
                a = torch.from_numpy(coef["a"]).to(self.device)
                pred = torch.empty(self.dim, dtype=torch.float32, device=self.device)
                with rnd._timed("lbfgs_predict", stream):
                    _lib.call("plato_agg_lbfgs_predict", self._table().data_ptr(), 2 * n, a.data_ptr(), coef["sigma"],
                              self.last_g.data_ptr(), v.data_ptr(), pred.data_ptr(), self.dim, h)
                nbytes = _lib.lib().plato_agg_delta_sqdist_workspace(k, n_f, n_i)
                work = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
                d2 = torch.zeros(k, dtype=torch.float64, device=self.device)
                with rnd._timed("delta_sqdist", stream):
                    _lib.call("plato_agg_delta_sqdist", *rnd._regions(tf, ti), k, *base_args, pred.data_ptr(), n_f, n_i,
                              work.data_ptr(), d2.data_ptr(), h)
                d2 = d2.cpu().numpy()  # stream-ordered, blocking: the scores are formed on the host
                now = list(normalised_distances(d2))
                scores = np.asarray([history_score(self.history.get(cid, ()), d) for cid, d in zip(received_ids, now)],
                                    dtype=np.float32)
                malicious, _ = two_means_1d(scores)
                info.update(distances=np.asarray(now, dtype=np.float32), scores=scores, malicious=malicious,
                            sigma=coef["sigma"], cond=coef["cond"], d2=d2, pred=(pred[:n_f], pred[n_f:]))
        except Exception:
            self._free.extend((y_new, s_new))
            raise
        # the round counted: extend the record and its Gram cache by the new row and column
        for cid, d in zip(received_ids, now):
            self.history.setdefault(cid, []).append(d)
        sy, ss = np.zeros((n + 1, n + 1)), np.zeros((n + 1, n + 1))
        sy[:n, :n], ss[:n, :n] = self.sy, self.ss
        sy[n, :n], sy[:n, n], sy[n, n] = dots[n:2 * n, 1], dots[:n, 2], dots[2 * n, 2]
        ss[n, :n] = ss[:n, n] = dots[:n, 1]
        ss[n, n] = dots[2 * n, 1]
        self.sy, self.ss, self.yy = sy, ss, np.append(self.yy, dots[2 * n + 1, 2])
        self.s_rows.append(s_new)
        self.y_rows.append(y_new)
        self._spare = [self.last_g, self.last_w]
        self.last_g, self.last_w = g, w_next
        self.rounds += 1
        self._trim()
        return info
