"""The reference of the diagonal log-domain forward score (include/ghmm.h, ghmm_logscore) on the cases of
logscore_cases.py, shared by test_logscore_host.py and test_logscore_gpu.py.  Plain numpy and the oracle, no
GPU, no tests.

    log b     oracle_lib.log_emission per stream in float64, folded over the streams by
              fullstreams_ref.fold(..., log=True) (the earlier streams' sum on the left)
    lattice   fulllogscore_ref.lattice in long double, its rounding bound fulllogscore_ref.lattice_bound

fulllogscore_ref.lattice forms all N x N terms of every step; beyond WIDE_REF states (the 512-state case:
80 s for its 600 frames) `lattice` below forms only the terms with a_ij > 0 instead, gathered per target
state, with fulllogscore_ref's own lse and log_transitions.  The terms left out are those lse masks to
-inf and adds as exact zeros, so the two agree to the long double's rounding (the sums pair up in another
order); test_logscore_host.test_gathered_lattice_is_the_reference_lattice holds them together on every
case, 1e-17 relative, five decades below the bound they are used under."""
import numpy as np

import fulllogscore_ref as LR
import oracle_lib as O
from fullcov_support import need_extended, offsets
from fullstreams_ref import fold

WIDE_REF = 128


def log_b(hms, Xs):
    """log b[F][N] of one word in float64: the oracle's log emission of every stream, added in stream order"""
    return fold([O.log_emission(hm, X) if len(X) else np.zeros((0, hm.N)) for hm, X in zip(hms, Xs)], log=True)


def gathered_lattice(A, logb, final_state, ft=np.longdouble, stats=None):
    """fulllogscore_ref.lattice with only the terms a_ij > 0 formed: the same values, the same stats"""
    if ft is np.longdouble:
        need_extended()
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[0]
    if len(logb) == 0:
        return ft(0)
    lb = np.asarray(logb).astype(ft).reshape(-1, N)
    with np.errstate(all="ignore"):
        terms, la_A = LR.log_transitions(A, ft)
        K = int(terms.sum(0).max())
        order = np.argsort(~terms, axis=0, kind="stable")[:K]       # [K][N]: column j's predecessors first
        j = np.arange(N)[None, :]
        mask, la_pred = terms[order, j], la_A[order, j]
        la = np.where(np.arange(N) == 0, ft(0), ft(-np.inf)) + lb[0]
        V = np.abs(la[np.isfinite(la)]).max(initial=0)
        for t in range(1, len(lb)):
            la = LR.lse(la[order] + la_pred, mask) + lb[t]
            V = max(V, np.abs(la[np.isfinite(la)]).max(initial=0))
        if stats is not None:
            stats["V"] = max(float(V), stats.get("V", 0.0))
            stats["La"] = max(float(np.abs(la_A).max()), stats.get("La", 0.0))
        return la[N - 1] if final_state else LR.lse(la)


def lattice(A, logb, final_state, ft=np.longdouble, stats=None):
    fn = gathered_lattice if np.asarray(A).shape[0] > WIDE_REF else LR.lattice
    return fn(A, logb, final_state, ft, stats)


def lattice_scores(A, logb, lens, final_state, ft=np.longdouble):
    """(scores[U] in ft, bound[U]): lattice() per utterance and fulllogscore_ref.lattice_bound with that
    utterance's own V and La (0 for T = 0)"""
    off = offsets(lens)
    N = np.asarray(A).shape[0]
    out, bound = [], []
    for u, T in enumerate(lens):
        st = {}
        out.append(lattice(A, logb[off[u]:off[u + 1]], final_state, ft, st))
        bound.append(LR.lattice_bound(int(T), N, st["V"], st["La"]) if T else 0.0)
    return np.array(out, dtype=ft), np.array(bound)


class Reference:
    """of a Case, computed once and left unchanged: logb[k] = word k's summed float64 log b[F][N_k],
    score[fs][K][U] the long-double lattice on it rounded to float64, score64[fs] the float64 lattice"""

    def __init__(self, case):
        self.logb = [log_b(hms, case.Xs) for hms in case.words]
        self.score, self.score_ld, self.score64 = {}, {}, {}
        for fs in (0, 1):
            ld = [lattice_scores(hms[0].A, lb, case.lens, fs)[0] for hms, lb in zip(case.words, self.logb)]
            self.score_ld[fs] = np.array(ld, dtype=np.longdouble)
            self.score[fs] = self.score_ld[fs].astype(np.float64)
            self.score64[fs] = np.array([lattice_scores(hms[0].A, lb, case.lens, fs, np.float64)[0]
                                         for hms, lb in zip(case.words, self.logb)])
        for a in list(self.score.values()) + list(self.score_ld.values()) + list(self.score64.values()) + self.logb:
            a.setflags(write=False)
