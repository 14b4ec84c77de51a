"""The cases of fullmstep_cases.py take the branches they are named for — host only.

test_fullmstep_gpu.py holds ghmm_mstep_full_dev to ghmm_mstep_full_host's bits on these cases; that
says nothing if a "quirk" case never reaches its quirk.  Here each one is checked on the HOST
M-step's output (and on the quotients updating_mix_param forms, restated by cases.new_cov): NaNs
where claimed, a determinant below 1e-20 before the split, the matrix unchanged where det == 0, and
so on.  Expected values are formed with the same IEEE operations in the same order, so they are
compared exactly unless a numpy inverse stands in for TFF's."""
import numpy as np
import pytest

import fullmstep_cases as K


def parts(G, name):
    hm, v, delta = K.build(G, name)
    nm, ncov = K.new_cov(v, hm.N, hm.M, hm.D)
    return hm, v, nm, ncov, K.host_result(G, name)


def test_case_table_covers_the_axes():
    shapes = list(K.PD.values())
    assert {s[2] for s in shapes} == {1, 2, 9, 47, 48}
    assert {s[0] for s in shapes} == {1, 6, 64}
    assert {s[1] for s in shapes} == {1, 2, 8, K.MCAP}
    assert {s[3] for s in shapes} == {0, 1, 2}


@pytest.mark.parametrize("name", list(K.PD))
def test_positive_definite_cases_are_plain(G, name):
    """no quirk: finite, every determinant >= 1 (B B' + I), the band of delta visible in A"""
    hm, v, nm, ncov, out = parts(G, name)
    delta = K.PD[name][3]
    for a in out.arrays():
        assert np.all(np.isfinite(a))
    assert np.all(out.det >= 1.0 - 1e-9)
    i, j = np.indices(out.A.shape)
    band = (j >= i) & (j <= i + delta)
    assert np.all(out.A[band] > 0.0) and np.all(out.A[~band] == 0.0)
    assert np.all(hm.A > 0.0)   # (the model before the step was dense)
    if hm.D > 1:
        k = (0, hm.M - 1)
        np.testing.assert_allclose(out.inv_cov[k] @ ncov[k], np.eye(hm.D), atol=1e-9)


def test_q1_skipped_state_is_inverted_twice(G):
    hm, v, nm, ncov, out = parts(G, "q1-den_c-zero")
    assert np.array_equal(out.mean[1], hm.mean[1])
    for k in range(hm.M):
        np.testing.assert_allclose(out.inv_cov[1, k], np.linalg.inv(hm.inv_cov[1, k]), rtol=1e-9, atol=1e-12)
        assert out.det[1, k] == pytest.approx(np.linalg.det(hm.inv_cov[1, k]), rel=1e-9)
        assert abs(out.det[1, k] / hm.det[1, k] - 1.0) > 1e-3      # not last iteration's det
    assert not np.array_equal(out.mean[0], hm.mean[0])              # the other states are updated
    hm, v, nm, ncov, out = parts(G, "q1-den_c-zero-d1")
    assert np.array_equal(out.det[0], hm.inv_cov[0, :, 0, 0])
    assert np.array_equal(out.inv_cov[0, :, 0, 0], 1.0 / hm.inv_cov[0, :, 0, 0])
    assert np.array_equal(out.mean[0], hm.mean[0])


def test_q2_rows_without_den_a_are_kept(G):
    hm, v, nm, ncov, out = parts(G, "q2-den_a-zero")
    for i in (0, 3):
        assert np.array_equal(out.A[i], hm.A[i]) and np.all(out.A[i] > 0.0)
    assert out.A[1, 0] == 0.0 and out.A[1, 3] == 0.0 and out.A[1, 1] > 0.0 and out.A[1, 2] > 0.0


def test_q3_zero_num_c_gives_nans_that_the_split_replaces(G):
    hm, v, nm, ncov, out = parts(G, "q3-num_c-zero")
    assert np.all(np.isnan(nm[1, 1])) and np.all(np.isnan(ncov[1, 1]))
    for a in out.arrays():
        assert np.all(np.isfinite(a))
    donor = 0 if np.linalg.det(ncov[1, 0]) > np.linalg.det(ncov[1, 2]) else 2
    assert np.array_equal(out.mean[1, 1], nm[1, donor] * 1.05)
    assert np.array_equal(out.mean[1, donor], nm[1, donor] * 0.95)
    assert np.array_equal(out.inv_cov[1, 1], out.inv_cov[1, donor]) and out.det[1, 1] == out.det[1, donor]
    assert out.c[1, 1] == out.c[1, donor]
    # M = 1: the Gaussian is its own donor and the NaNs stay
    hm, v, nm, ncov, out = parts(G, "q3-num_c-zero-m1")
    assert np.all(np.isnan(out.mean[1, 0])) and np.all(np.isnan(out.inv_cov[1, 0]))
    assert out.det[1, 0] == 0.0 and out.c[1, 0] == 1.0
    assert np.all(np.isfinite(out.mean[0])) and np.all(np.isfinite(out.inv_cov[0]))
    assert "q3-num_c-zero-m1" in K.NAN_CASES


def test_nan_cases_are_listed(G):
    for name in K.QUIRKS:
        out = K.host_result(G, name)
        has = any(np.isnan(a).any() for a in out.arrays())
        assert has == (name in K.NAN_CASES), name


def test_q4_zero_det_leaves_the_matrix(G):
    hm, v, nm, ncov, out = parts(G, "q4-singular-m1")
    sing = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 1.0], [0.0, 1.0, 1.0]])
    assert np.array_equal(ncov[0, 0], sing)
    assert out.det[0, 0] == 0.0
    assert np.array_equal(out.inv_cov[0, 0], sing)                  # un-inverted, then copied onto itself
    assert np.array_equal(out.mean[0, 0], nm[0, 0] * 1.05 * 0.95)
    hm, v, nm, ncov, out = parts(G, "q4-singular-m2")
    assert out.det[0, 0] == out.det[0, 1] != 0.0
    assert np.array_equal(out.inv_cov[0, 0], out.inv_cov[0, 1])
    assert np.array_equal(out.mean[0, 0], nm[0, 1] * 1.05)


def test_q5_donor_order_and_modified_donor(G):
    hm, v, nm, ncov, out = parts(G, "q5-two-small-dets")
    dets = np.linalg.det(ncov[1])
    assert dets[0] < K.ZERO_DET and dets[2] < K.ZERO_DET and dets[1] > 1e-3
    assert np.array_equal(ncov[1, 1], ncov[1, 3])                   # equal keys: the order is sorting's
    assert not np.array_equal(nm[1, 1], nm[1, 3])
    assert np.array_equal(out.mean[1, 0], nm[1, 1] * 1.05) and np.array_equal(out.mean[1, 1], nm[1, 1] * 0.95)
    assert np.array_equal(out.mean[1, 2], nm[1, 3] * 1.05) and np.array_equal(out.mean[1, 3], nm[1, 3] * 0.95)
    assert np.all(out.det[1] == out.det[1, 1])
    hm, v, nm, ncov, out = parts(G, "q5-donor-modified")
    dets = np.prod(np.diagonal(ncov[0], axis1=-2, axis2=-1), axis=-1)
    assert np.linalg.det(ncov[0, 1]) > 1e-3 and dets[3] > dets[0] > dets[2] and dets[3] < K.ZERO_DET
    assert np.array_equal(out.mean[0, 1], nm[0, 1] * 0.95)
    assert np.array_equal(out.mean[0, 0], nm[0, 1] * 1.05 * 0.95)   # received, then gave to 3
    assert np.array_equal(out.mean[0, 3], nm[0, 1] * 1.05 * 1.05)   # from the rewritten Gaussian 0
    assert np.array_equal(out.mean[0, 2], nm[0, 3] * 1.05)          # from 3 while it was still small
    assert out.det[0, 2] < K.ZERO_DET and out.det[0, 3] == out.det[0, 0] == out.det[0, 1] > 1e-3
    assert np.array_equal(out.inv_cov[0, 3], out.inv_cov[0, 1])


def test_q6_single_gaussian_is_split_with_itself(G):
    hm, v, nm, ncov, out = parts(G, "q6-self-split")
    assert out.det[2, 0] < K.ZERO_DET and out.det[2, 0] > 0.0
    assert np.array_equal(out.mean[2, 0], nm[2, 0] * 1.05 * 0.95)
    assert np.array_equal(out.mean[1, 0], nm[1, 0])
    assert np.all(out.c == 1.0)


def test_q7_floors(G):
    hm, v, nm, ncov, out = parts(G, "q7-small-weights")
    N, M = hm.N, hm.M
    st = v[N * N + N:N * N + 2 * N], v[N * N + 2 * N:N * N + 2 * N + N * M].reshape(N, M)
    raw = st[1] / st[0][:, None]
    assert (raw < K.FLOOR).sum() == 3
    for i in range(N):
        c = [max(float(x), K.FLOOR) for x in raw[i]]
        for _ in range(2):      # changing_zero_coef, then treat_zero_det's renormalisation
            s = 0.0
            for x in c:
                s += x
            c = [x / s for x in c]
        assert np.array_equal(out.c[i], np.array(c))
    hm, v, nm, ncov, out = parts(G, "q7-floored-diagonal")
    d = np.diagonal(ncov[1, 0])
    assert d[0] < K.FLOOR and d[2] < K.FLOOR
    assert out.det[1, 0] == pytest.approx(K.FLOOR * 0.5 * K.FLOOR, rel=1e-12)
    np.testing.assert_allclose(np.diagonal(out.inv_cov[1, 0]), [1e5, 2.0, 1e5, 1.0], rtol=1e-12)


def test_q8_negative_pivot_gives_a_negative_det(G):
    hm, v, nm, ncov, out = parts(G, "q8-negative-det")
    assert out.det[0, 0] < 0.0 and out.det[1, 0] > 0.0
    assert out.det[0, 0] == pytest.approx(np.linalg.det(ncov[0, 0]), rel=1e-9)
    np.testing.assert_allclose(out.inv_cov[0, 0], np.linalg.inv(ncov[0, 0]), rtol=1e-9, atol=1e-12)
    hm, v, nm, ncov, out = parts(G, "q8-negative-det-m2")
    assert np.all(out.det[0] < 0.0) and np.all(out.det[1] > 0.0)
