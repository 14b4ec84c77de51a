"""Cases for the diagonal M-step on the device (ghmm_mstep): a HostModel (the model before the step),
a small corpus and a HAND-EDITED statistics vector, so that every branch of the reference's M-step
(TF:332-346, TF:1338-1359, TF:1862-1955) and every code path of the device's can be aimed at.

Shared by test_mstep_host.py, which asserts on the oracle's result that each case reaches what it is
named for, and by test_mstep_gpu.py, which holds ghmm_mstep to the expected model's bits and then
looks at the state the step derives (which ghmm_model_get does not show) through the calls that
read it.  numpy and the oracle, no GPU; every case and its expected model are computed once.

A case = name + shape (N, M, D).  Model and corpus: streams_util.synth_case; base vector:
O.estep(hm, X, lens, delta)[0]; then the edit of the name (EDITS below).  `finite`: the model after
the step has no NaN / inf parameter and no det == 0 — only those cases get the follow-up calls.

Which kernel takes a shape.  ghmm_model_create (csrc/ghmm_hip.hip) decides the matrix-core form:
    Mp = M rounded up to a power of two (M <= 16) or to a multiple of 16;  tps = max(Mp / 16, 1)
    NT = ceil(N Mp / 16);  DP = (D + 1) rounded up to a multiple of 4
    per_tile = DP / 2 * 64 * 8 bytes;  slabs = 8 waves * 16 * (2 DP + 1) * 8 bytes
    tcmax = min((150 KiB - slabs) / per_tile, 6);  TC = min(tcmax / tps * tps, NT)
    mfma_ok = TC >= tps and TC > 0 and TC per_tile + slabs <= 150 KiB and D <= 64
ghmm_mstep then launches k_mstep_mfma when mfma_ok, else k_mstep; mstep_state inside either stages
the state in LDS when (M D + M) * 8 <= 56 KiB and goes through global memory otherwise (every
matrix-core shape is far below that: M <= 96, D <= 63).  geometry() restates this; PATHS is checked
against it at import, and test_mstep_gpu.py checks the matrix-core half on the device."""
import functools
from collections import namedtuple

import numpy as np

import oracle_lib as O
from streams_util import synth_case

FLOOR = 1.0e-5      # FINITE_PROBAB, TF:39
COND_MAX = 1.0e4    # csrc/ghmm_mfma.hpp: above it a Gaussian leaves the expanded forms


def geometry(N, M, D):
    """(mfma_ok, Mp, NT, DP, TC, np) as ghmm_model_create and k_mstep_mfma form them"""
    Mp = 1
    if M <= 16:
        while Mp < M:
            Mp <<= 1
    else:
        Mp = (M + 15) // 16 * 16
    tps = Mp // 16 if Mp > 16 else 1
    NT = (N * Mp + 15) // 16
    DP = (D + 1 + 3) // 4 * 4
    per_tile = DP // 2 * 64 * 8
    slabs = 8 * 16 * (2 * DP + 1) * 8
    if D > 64 or slabs >= 150 * 1024:
        return False, Mp, NT, DP, 0, 512 // DP
    TC = min(min((150 * 1024 - slabs) // per_tile, 6) // tps * tps, NT)
    ok = TC >= tps and TC > 0 and TC * per_tile + slabs <= 150 * 1024
    return ok, Mp, NT, DP, TC, 512 // DP


def path_of(N, M, D):
    if geometry(N, M, D)[0]:
        return "mfma"
    return "lds" if (M * D + M) * 8 <= 56 * 1024 else "global"


QUIRK_SHAPES = ((5, 3, 5), (10, 8, 39))
# shape -> path.  Derivation (geometry above):
#   (13, 8, 39)  DP 40: np = 512 / 40 = 12 column parts; G = 104 > 8 * 12 = 96: the unrolled oglob
#                loop runs a second round whose indices are clamped
#   (3, 20, 13)  Mp 32, tps 2: a state spans two tiles; DP 16: tcmax 6, TC 6
#   (2, 96, 13)  Mp 96, tps 6 = tcmax = TC: the widest mixture count that takes the form
#   (2, 97, 13)  Mp 112, tps 7 > tcmax 6: TC 0;  97 * 14 = 1358 doubles: LDS
#   (3, 2, 63)   DP 64: slabs 132 096, per_tile 16 384: tcmax 1 = TC (NT 1): the largest D
#   (3, 2, 64)   DP 68: slabs 140 288, per_tile 17 408 > 13 312 left: tcmax 0
#   (2, 112, 63) Mp 112, tps 7 > tcmax 1; 112 * 64 = 7168 doubles = 56 KiB exactly: LDS, at the edge
#   (2, 112, 64) D = 64 takes no tile; 112 * 65 = 7280 > 7168: global
#   (2, 184, 39) Mp 192, tps 12 > 6; 184 * 40 = 7360 > 7168: global
PATHS = {(13, 8, 39): "mfma", (3, 20, 13): "mfma", (2, 96, 13): "mfma", (2, 97, 13): "lds",
         (3, 2, 63): "mfma", (3, 2, 64): "lds", (2, 112, 63): "lds", (2, 112, 64): "global",
         (2, 184, 39): "global"}
for _s, _p in PATHS.items():
    assert path_of(*_s) == _p, (_s, _p, path_of(*_s))
for _s in QUIRK_SHAPES:
    assert path_of(*_s) == "mfma", _s
assert (112 * 63 + 112) * 8 == 56 * 1024 and (112 * 64 + 112) * 8 > 56 * 1024
assert geometry(13, 8, 39)[5] == 12 and 13 * 8 > 8 * 12 and (13 * 8) % 12 != 0
assert geometry(5, 3, 5)[1:4] == (4, 2, 8) and geometry(3, 20, 13)[1] == 32
assert geometry(2, 96, 13)[4] == 6 and geometry(3, 2, 63)[3:5] == (64, 1)

# name -> (finite, delta, dense start).  The edits themselves: _edit.
EDITS = {
    "plain": (True, 1, False),
    "row-kept": (True, 1, True),            # (a dense start: the kept row HAS entries outside the band)
    "state-skipped": (True, 1, False),
    "nothing-updated": (True, 1, False),
    "weight-floor": (False, 1, False),
    "weight-floor-finite": (True, 1, False),
    "var-floor-all": (True, 1, False),
    "var-negative": (True, 1, False),
    "narrow-one-coefficient": (True, 1, False),
    "det-overflow": (False, 1, False),
    "delta2": (True, 2, True),
    "band-dirty-delta2": (True, 2, True),
    "nan-in-one-state": (False, 1, False),
    "det-subnormal": (True, 1, False),
}
PATH_EDITS = ("plain", "state-skipped", "var-floor-all")

KEPT_ROW = 1        # row-kept
SKIPPED = 1         # state-skipped
WF_STATE, WF_TINY, WF_ZERO = 3, 0, 1    # weight-floor: Gaussians (3, 0) and (3, 1)
NEG = (1, 1, 2)     # var-negative
NARROW = (2, 0, 3)  # narrow-one-coefficient
OVER = (2, 1)       # det-overflow
NAN_G = (3, 1)      # nan-in-one-state
SUBNORMAL = (0, 1)  # det-subnormal


def floored_gaussian(N, M):
    """var-floor-all's Gaussian: at (5, 3, 5) state 1 sits in tile 0, which four states' blocks share.
    (At D = 63 and 64 the oracle's E-step on the stepped model stays finite with this one; with some
    others a frame's b underflows to 0 and the reference's 0/0 takes the whole vector.)"""
    return 1, 0


def case_id(name, shape):
    return f"{name}-{shape[0]}x{shape[1]}x{shape[2]}"


CASES = {}          # id -> (name, shape)
for _shape in QUIRK_SHAPES:
    for _name in EDITS:
        if _name == "det-subnormal" or (_name == "det-overflow" and _shape != QUIRK_SHAPES[0]):
            continue
        CASES[case_id(_name, _shape)] = (_name, _shape)
for _shape in PATHS:
    for _name in PATH_EDITS:
        CASES[case_id(_name, _shape)] = (_name, _shape)
CASES[case_id("det-subnormal", (3, 2, 64))] = ("det-subnormal", (3, 2, 64))
ALL = tuple(CASES)
FINITE = tuple(k for k in ALL if EDITS[CASES[k][0]][0])
MFMA = tuple(k for k in ALL if path_of(*CASES[k][1]) == "mfma")

Case = namedtuple("Case", "name shape hm X lens v delta finite")


def lens_of(N):
    """three utterances of a few dozen frames, every T >= N"""
    return [37, 20, max(12, N)]


def _edit(name, hm, s, N, M, D):
    """the edit of `name` on the views s = G.split_stats(v) of the base vector"""
    if name in ("plain", "delta2"):
        pass
    elif name == "row-kept":
        s["den_a"][KEPT_ROW] = 0.0
    elif name == "state-skipped":
        s["den_c"][SKIPPED] = 0.0
    elif name == "nothing-updated":
        s["den_c"][:] = 0.0
        s["den_a"][:] = 0.0
        s["num_c"][:] = 0.0
    elif name in ("weight-floor", "weight-floor-finite"):
        # a tiny weight whose Gaussian keeps its mean and variances (both sums scaled with num_c)
        i, k = WF_STATE, WF_TINY
        mean, var = s["num_mu"][i, k] / s["num_c"][i, k], s["num_var"][i, k] / s["num_c"][i, k]
        s["num_c"][i, k] = 1e-9 * s["den_c"][i]
        s["num_mu"][i, k] = mean * s["num_c"][i, k]
        s["num_var"][i, k] = var * s["num_c"][i, k]
        if name == "weight-floor":
            s["num_c"][i, WF_ZERO] = 0.0
            s["num_mu"][i, WF_ZERO] = 0.0
            s["num_var"][i, WF_ZERO] = 0.0
    elif name in ("var-floor-all", "det-subnormal"):
        i, k = SUBNORMAL if name == "det-subnormal" else floored_gaussian(N, M)
        s["num_var"][i, k] = 1e-9 * s["num_c"][i, k]
    elif name == "var-negative":
        s["num_var"][NEG] = -3e-13
    elif name == "narrow-one-coefficient":
        i, k, d = NARROW
        centre = s["num_mu"][:, :, d].sum() / s["num_c"].sum()
        s["num_var"][i, k, d] = 1e-4 * s["num_c"][i, k]
        s["num_mu"][i, k, d] = (centre + 3.0) * s["num_c"][i, k]
    elif name == "det-overflow":
        s["num_var"][OVER] = 1e300
    elif name == "band-dirty-delta2":
        s["num_a"][np.tril_indices(N, -1)] = 0.37
        s["num_a"][np.triu_indices(N, 3)] = 0.37
    elif name == "nan-in-one-state":
        s["num_mu"][NAN_G] = np.nan
    else:
        raise KeyError(name)


@functools.lru_cache(maxsize=None)
def build(G, cid):
    """the Case of an id, computed once; callers leave its arrays unchanged"""
    name, (N, M, D) = CASES[cid]
    finite, delta, dense = EDITS[name]
    hm, X, lens = synth_case(G, N, M, D, lens_of(N), dense_A=dense)
    v = O.estep(hm, X, lens, delta=delta, dumps=False)[0].copy()
    base = G.split_stats(v, N, M, D)     # views into v (the layout of include/ghmm.h)
    assert np.all(np.isfinite(v)) and np.all(base["den_a"] > 0.0) and np.all(base["den_c"] > 0.0) \
        and np.all(base["num_c"] > 0.0), cid
    _edit(name, hm, base, N, M, D)
    return Case(name, (N, M, D), hm, X, lens, v, delta, finite)


def band(N, delta):
    i, j = np.indices((N, N))
    return (j >= i) & (j <= i + delta)


def mask_band(new, v, delta):
    """ghmm_mstep's contract (include/ghmm.h): in every row it updates (den_a != 0), a_ij outside
    i <= j <= i + delta is +0.0 whatever num_a holds there; orc_update_trans does not mask"""
    N = new.N
    den_a = v[N * N:N * N + N]
    out = ~band(N, delta) & (den_a != 0.0)[:, None]
    new.A[out] = 0.0
    return new


@functools.lru_cache(maxsize=None)
def expected(G, cid):
    """the model ghmm_mstep must produce, bit for bit: O.mstep, masked to the band"""
    c = build(G, cid)
    with np.errstate(all="ignore"):
        return mask_band(O.mstep(c.hm, c.v), c.v, c.delta)


def is_finite_model(hm):
    return all(np.all(np.isfinite(a)) for a in hm.arrays()) and bool(np.all(hm.det != 0.0))


@functools.lru_cache(maxsize=None)
def follow_up(G, cid):
    """whether the case gets the calls on the stepped model: its `finite` flag; det-subnormal only if
    the oracle's own E-step on the expected model is finite as well"""
    c = build(G, cid)
    if not c.finite:
        return False
    if c.name == "det-subnormal":
        with np.errstate(all="ignore"):
            return bool(np.all(np.isfinite(O.estep(expected(G, cid), c.X, c.lens, delta=c.delta, dumps=False)[0])))
    return True
