"""The full-covariance .hmm format (reader RC:591-707 of the reference's full-covariance
recogniser) — host code only, no GPU.  tests/golden/full_cov_models/ holds the 13 models the
reference ships (test/test/models, 32-bit build: 4-byte length prefix)."""
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN

MDIR = os.path.join(GOLDEN, "full_cov_models")
FILES = sorted(f for f in os.listdir(MDIR) if f.endswith(".hmm"))


def decode(raw, lb):
    """An independent decode of a one-stream full-covariance .hmm with an lb-byte length prefix."""
    n = int.from_bytes(raw[:lb], "little")
    o = lb
    word = raw[o:o + n].decode()
    o += n
    N, P, M, D = struct.unpack_from("<4i", raw, o)
    o += 16
    assert P == 1
    v = np.frombuffer(raw, dtype="<f8", offset=o)
    A = v[:N * N].reshape(N, N)
    k = N * N
    c = np.empty((N, M)); mean = np.empty((N, M, D)); det = np.empty((N, M)); ic = np.empty((N, M, D, D))
    for i in range(N):
        c[i] = v[k:k + M]
        k += M
        for m in range(M):
            mean[i, m] = v[k:k + D]
            det[i, m] = v[k + D]
            ic[i, m] = v[k + D + 1:k + D + 1 + D * D].reshape(D, D)
            k += D + 1 + D * D
    assert k == len(v)
    return word, A, c, mean, det, ic


@pytest.mark.parametrize("fn", FILES)
def test_shipped_models_read(G, fn):
    assert len(FILES) == 13
    path = os.path.join(MDIR, fn)
    hm = G.HostFullModel.read(path)
    word, A, c, mean, det, ic = decode(open(path, "rb").read(), 4)
    assert hm.word == word == fn[len("mean_"):-len(".hmm")]
    assert (hm.N, hm.M, hm.D) == (6, 1, 9)
    for got, ref in ((hm.A, A), (hm.c, c), (hm.mean, mean), (hm.det, det), (hm.inv_cov, ic)):
        assert np.array_equal(got, ref)
    # det and the inverse covariance in their own slots: a covariance determinant is positive,
    # an inverse covariance is symmetric with a positive diagonal, and det * det(inv_cov) = 1
    assert (hm.det > 0).all()
    assert np.allclose(hm.inv_cov, np.swapaxes(hm.inv_cov, -1, -2), rtol=1e-6, atol=1e-12)
    assert (np.diagonal(hm.inv_cov, axis1=-2, axis2=-1) > 0).all()
    assert np.allclose(hm.det * np.linalg.det(hm.inv_cov), 1.0, rtol=1e-6)
    # transitions: rows of A are distributions
    assert np.allclose(hm.A.sum(1), 1.0)


@pytest.mark.parametrize("fn", FILES)
def test_write_reproduces_shipped_bytes(G, fn, tmp_path):
    path = os.path.join(MDIR, fn)
    hm = G.HostFullModel.read(path)
    out4 = str(tmp_path / "m4.hmm")
    hm.write(out4, 4)
    assert open(out4, "rb").read() == open(path, "rb").read()
    out8 = str(tmp_path / "m8.hmm")
    hm.write(out8, 8)
    assert os.path.getsize(out8) == os.path.getsize(path) + 4
    back = G.HostFullModel.read(out8)
    assert back.word == hm.word
    for a, b in zip(back.arrays(), hm.arrays()):
        assert np.array_equal(a, b)


def test_full_reader_refuses_diagonal_and_several_streams(G, tmp_path):
    rng = np.random.default_rng(5)
    N, M, D = 4, 2, 3
    hd = G.HostModel(np.eye(N), np.full((N, M), 0.5), rng.normal(size=(N, M, D)),
                     rng.uniform(0.5, 2, (N, M, D)), rng.uniform(0.5, 2, (N, M)), word="diag")
    for lb in (4, 8):
        p = str(tmp_path / f"diag{lb}.hmm")
        hd.write(p, lb)
        with pytest.raises(G.GhmmError) as e:
            G.HostFullModel.read(p)
        assert e.value.code == G.ERR_FORMAT
    # two streams in the full-covariance layout
    word = b"two"
    Ms, Ds = (2, 1), (3, 2)
    raw = len(word).to_bytes(8, "little") + word + struct.pack("<2i", N, 2) + struct.pack("<4i", *Ms, *Ds)
    raw += np.eye(N).tobytes()
    for M_, D_ in zip(Ms, Ds):
        raw += np.ones(N * (M_ + M_ * (D_ * D_ + D_ + 1))).tobytes()
    p = str(tmp_path / "p2.hmm")
    open(p, "wb").write(raw)
    with pytest.raises(G.GhmmError) as e:
        G.HostFullModel.read(p)
    assert e.value.code == G.ERR_UNSUPPORTED
    # truncated by one byte: neither header width fits
    open(p, "wb").write(open(os.path.join(MDIR, FILES[0]), "rb").read()[:-1])
    with pytest.raises(G.GhmmError) as e:
        G.HostFullModel.read(p)
    assert e.value.code == G.ERR_FORMAT
