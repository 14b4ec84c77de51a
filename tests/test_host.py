"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol of
include/ghmm.h, the host-side file formats and initial-model construction match the
reference, the synthetic generator is deterministic, and the product refuses to run
the hot path without a GPU (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from _load import PKG_DIR, ROOT


def test_abi_library_exports_every_declared_symbol(G):
    lib = ctypes.CDLL(G.HIP_LIB)
    hdr = open(os.path.join(ROOT, "include", "ghmm.h")).read()
    declared = set(re.findall(r"\b(ghmm_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"ghmm_ctx", "ghmm_model", "ghmm_corpus", "ghmm_stats", "ghmm_host_model", "ghmm_comm"}
    assert len(declared) >= 57
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/ghmm.h but not exported"
    assert set(G.SYMBOLS) == declared
    assert lib.ghmm_version() == 200


def test_no_cpu_fallback(G, tmp_path):
    """Without a device the hot path must fail loudly, never compute on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(G.GhmmError) as e:
        G.Context(0)
    assert e.value.code == G.ERR_NODEVICE
    exe = os.path.join(PKG_DIR, "bin", "hmm-continuous-train-fs")
    lst = os.path.join(GOLDEN, "perfil", "mean_vc_186_f_03_ap_0225.perfil")
    p = subprocess.run([exe, "w", "6", "1", "1", "/dev/stdin", str(tmp_path / "nogpu.hmm")],
                       input=(lst + "\n").encode(), stdout=subprocess.PIPE)
    assert p.returncode == 1 and b"GPU context" in p.stdout


def test_product_does_not_touch_the_oracle():
    """The oracle is test infrastructure: nothing under the package or include/ may include,
    link, dlopen or import it (comments may mention it).  The one dlopen in the product loads
    RCCL for the statistics all-reduce (ghmm_comm_*): every shared-object name the library
    can pass to it must be an RCCL name."""
    import re
    bad = re.compile(r'libghmm_oracle|oracle_lib|#\s*include\s*[<"][^>"]*oracle|orc_[a-z_]+\s*\(')
    for root in (PKG_DIR, os.path.join(ROOT, "include")):
        for d, _, files in os.walk(root):
            for fn in files:
                if fn.endswith((".c", ".hip", ".hpp", ".h", ".py")) or fn == "Makefile":
                    txt = open(os.path.join(d, fn), errors="replace").read()
                    assert not bad.search(txt), f"{fn} reaches into oracle/"
                    if "dlopen" in txt:
                        assert fn == "ghmm_hip.hip", f"{fn} calls dlopen"
                        sonames = re.findall(r'"([^"\n]*\.so[^"\n]*)"', txt)
                        assert sonames and all("rccl" in n for n in sonames), sonames
                        assert re.findall(r'getenv\("([A-Z_]+)"\)', txt) == ["GHMM_RCCL_LIB"]
    out = subprocess.run(["ldd", os.path.join(PKG_DIR, "libghmm_hip.so")], stdout=subprocess.PIPE)
    assert b"ghmm_oracle" not in out.stdout
    for exe in ("hmm-continuous-train-fs", "recognition-continuous-test-fs"):
        out = subprocess.run(["ldd", os.path.join(PKG_DIR, "bin", exe)], stdout=subprocess.PIPE)
        assert b"ghmm_oracle" not in out.stdout and b"libghmm_hip" in out.stdout


def test_command_line_usage(G):
    for exe, first in (("hmm-continuous-train-fs", b"Usage: hmm_continuous_fs"),
                       ("recognition-continuous-test-fs", b"Usage: recognition_continuous_fs")):
        p = subprocess.run([os.path.join(PKG_DIR, "bin", exe), "a", "b"], stdout=subprocess.PIPE)
        assert p.returncode == 1 and p.stdout.startswith(first)


def test_perfil_roundtrip_and_bundled_files(G, tmp_path):
    X = np.random.default_rng(0).normal(size=(17, 9))
    p = str(tmp_path / "a.perfil")
    G.perfil_write(p, X)
    raw = open(p, "rb").read()
    assert len(raw) == 4 + 17 * 9 * 8 and int.from_bytes(raw[:4], "little") == 9
    assert np.array_equal(G.perfil_read(p), X)
    # the reference's bundled utterances: 9-d, 103..213 frames
    frames = []
    for fn in sorted(os.listdir(os.path.join(GOLDEN, "perfil"))):
        Y = G.perfil_read(os.path.join(GOLDEN, "perfil", fn))
        assert Y.shape[1] == 9
        frames.append(Y.shape[0])
    assert len(frames) == 13 and min(frames) == 103 and max(frames) == 213
    with pytest.raises(G.GhmmError) as e:
        G.perfil_read(str(tmp_path / "missing.perfil"))
    assert e.value.code == G.ERR_IO
    open(str(tmp_path / "bad.perfil"), "wb").write(b"\0\0")
    with pytest.raises(G.GhmmError) as e:
        G.perfil_read(str(tmp_path / "bad.perfil"))
    assert e.value.code == G.ERR_FORMAT


def test_hmm_file_both_header_widths(G, load_case, tmp_path):
    hm = load_case("bundled13_m3").model0
    hm.word = "vc_186_f_03_ap_0225"
    for lb in (8, 4):
        p = str(tmp_path / f"m{lb}.hmm")
        hm.write(p, lb)
        N, M, D = hm.N, hm.M, hm.D
        # layout of writing_model, TF:2043-2146
        assert os.path.getsize(p) == lb + len(hm.word) + 16 + 8 * (N * N + N * (M + M * (2 * D + 1)))
        back = G.HostModel.read(p)
        assert back.word == hm.word and (back.N, back.M, back.D) == (N, M, D)
        for a, b in zip(back.arrays(), hm.arrays()):
            assert np.array_equal(a, b)
    # a 64-bit build of the reference writes exactly the 8-byte form: byte-compare with the
    # golden model the real trainer wrote (re-serialised from its parsed content)
    open(str(tmp_path / "junk.hmm"), "wb").write(b"\x07" * 100)
    with pytest.raises(G.GhmmError) as e:
        G.HostModel.read(str(tmp_path / "junk.hmm"))
    assert e.value.code == G.ERR_FORMAT


def test_shipped_full_covariance_models_are_refused_not_misread(G):
    """The 13 .hmm files the reference ships were written by its FULL-covariance trainer on
    a 32-bit build: the diagonal reader must say 'bad format', not parse
    garbage.  (tests/golden/full_cov_models/: the reference's test/test/models/*.hmm verbatim.)"""
    d = os.path.join(GOLDEN, "full_cov_models")
    files = [f for f in sorted(os.listdir(d)) if f.endswith(".hmm")]
    assert len(files) == 13
    for fn in files:
        word = fn[len("mean_"):-len(".hmm")]
        # 4-byte length + word + 4 ints + A[6][6] + 6 x (1 weight + 9 means + det + 9x9 inverse)
        assert os.path.getsize(os.path.join(d, fn)) == 4 + len(word) + 16 + 8 * (36 + 6 * 92)
        with pytest.raises(G.GhmmError) as e:
            G.HostModel.read(os.path.join(d, fn))
        assert e.value.code == G.ERR_FORMAT


@pytest.mark.parametrize("name", ["bundled186_m1", "bundled13_m3", "synth39_m8_refinit"])
def test_initial_model_is_bit_exact_vs_reference(G, load_case, name):
    """creating_initial_model TF:732-1317 (uniform segmentation, LBG, k-means, variance
    floor) — including the needle components of the 39-d case (det = 1e-195)."""
    c = load_case(name)
    hm = G.HostModel.init_from(c.X, c.lens, c.N, c.M)
    for a, b in zip(hm.arrays(), c.model0.arrays()):
        assert np.array_equal(a, b, equal_nan=True)


def test_synthetic_generator_is_deterministic_and_shardable(G):
    mean, std = G.synth_truth(10, 8, 39)
    m2, s2 = G.synth_truth(10, 8, 39)
    assert np.array_equal(mean, m2) and np.array_equal(std, s2)
    assert 0.5 <= std.min() and std.max() <= 1.5 and abs(mean.std() - 2.0) < 0.1
    lens = np.array([50, 60, 70, 80], dtype=np.int32)
    X = G.synth_utterances(mean, std, lens)
    # shards of the same corpus generated independently (what each rank does)
    Xa = G.synth_utterances(mean, std, lens[:2], first_utt=0)
    Xb = G.synth_utterances(mean, std, lens[2:], first_utt=2)
    assert np.array_equal(X, np.concatenate([Xa, Xb]))
    hm = G.synth_start_model(mean, std, 0.05)
    assert np.allclose(hm.A.sum(1), 1.0) and np.allclose(hm.c.sum(1), 1.0)
    assert np.allclose(hm.det, np.prod(1.0 / hm.inv_var, axis=2), rtol=1e-12)


def test_stats_layout_matches_header(G):
    v = np.arange(G.stats_len(3, 2, 4), dtype=np.float64)
    s = G.split_stats(v, 3, 2, 4)
    assert s["num_a"].shape == (3, 3) and s["num_mu"].shape == (3, 2, 4)
    assert s["loglik"] == v[-2] and s["n_utt"] == v[-1]
    assert G.stats_len(10, 8, 39) == 6442 and G.stats_len(10, 64, 39) == 50682


def test_length_balanced_shards(G):
    """ghmm_shard_balanced (C, used by the trainer's rank mode) = em.shard_balanced (bench /
    torch path): sort by length, deal in turn; every utterance lands on exactly
    one rank and the ranks' frame counts differ by at most the longest utterance."""
    from _load import load_pkg
    em = load_pkg().em
    rng = np.random.default_rng(0)
    for n in (0, 1, 5, 17, 1000):
        lens = rng.integers(1, 500, n).astype(np.int32)
        for world in (1, 2, 3, 8):
            seen, frames = [], []
            for r in range(world):
                a = list(G.shard_balanced(lens, r, world))
                assert a == em.shard_balanced(lens, r, world) and a == sorted(a)
                seen += a
                frames.append(int(lens[a].sum()))
            assert sorted(seen) == list(range(n))
            if n:
                assert max(frames) - min(frames) <= lens.max()
    # equal lengths: contiguous-free but equal counts
    assert [len(G.shard_balanced(np.full(1000, 300), r, 8)) for r in range(8)] == [125] * 8


def test_perfil_stat_reads_header_and_size(G, tmp_path):
    X = np.arange(35.0).reshape(7, 5)
    p = os.path.join(str(tmp_path), "a.perfil")
    G.perfil_write(p, X)
    assert G.perfil_stat(p) == (5, 7)
    D, T = G.perfil_stat(os.path.join(GOLDEN, "perfil", "mean_vc_186_f_03_ap_0225.perfil"))
    assert D == 9 and T == len(G.perfil_read(os.path.join(GOLDEN, "perfil", "mean_vc_186_f_03_ap_0225.perfil")))
    with pytest.raises(G.GhmmError):
        G.perfil_stat(os.path.join(str(tmp_path), "missing.perfil"))


# ------------------------------------------- rendezvous file protocol (ghmm_rendezvous.c)

def _rdv_proc(path, rank, world, timeout, id_bytes, delay, q):
    import time
    from _load import ghmm
    G = ghmm()
    time.sleep(delay)
    try:
        q.put((rank, G.rendezvous_file(path, rank, world, timeout, id_bytes), None))
    except G.GhmmError as e:
        q.put((rank, None, e.code))


def _rdv_threads(G, path, world, timeout, ident, delays=None, absent=()):
    """one thread per rank (the C call releases the GIL, keeps no global state)"""
    import threading
    import time
    res = {}

    def run(r):
        time.sleep((delays or {}).get(r, 0.0))
        try:
            res[r] = G.rendezvous_file(path, r, world, timeout, ident if r == 0 else None)
        except G.GhmmError as e:
            res[r] = e.code
    ts = [threading.Thread(target=run, args=(r,)) for r in range(world) if r not in absent]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return res


def test_rendezvous_three_processes_and_a_late_rank_zero(G, tmp_path):
    """The id exchange of ghmm_comm_create_file with more than one rank, as
    separate PROCESSES: every rank obtains rank 0's 128 bytes, a rank 0 that starts late is
    waited for, and nothing is left behind."""
    import multiprocessing as mp
    ident = bytes(range(128))
    path = str(tmp_path / "job.id")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rdv_proc, args=(path, r, 3, 30.0, ident if r == 0 else None,
                                                 0.6 if r == 0 else 0.0, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=60) for _ in procs)
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    assert [r[0] for r in res] == [0, 1, 2]
    assert all(r[1] == ident and r[2] is None for r in res)
    assert os.listdir(tmp_path) == []


def test_rendezvous_timeouts_and_stale_files(G, tmp_path):
    ident = bytes((7 * k + 3) % 256 for k in range(128))
    # world = 1: nothing to exchange, nothing written
    path = str(tmp_path / "one.id")
    assert G.rendezvous_file(path, 0, 1, 1.0, ident) == ident and os.listdir(tmp_path) == []
    # rank 0 never comes: the other rank gives up with GHMM_ERR_IO and takes its join file away
    path = str(tmp_path / "a.id")
    assert _rdv_threads(G, path, 2, 0.3, ident, absent=(0,)) == {1: G.ERR_IO}
    assert os.listdir(tmp_path) == []
    # rank 2 never comes: the id is published only once EVERY rank has announced itself, so
    # ranks 0 and 1 both give up (nobody is left holding an id of a job that cannot start)
    path = str(tmp_path / "b.id")
    res = _rdv_threads(G, path, 3, 0.4, ident, absent=(2,))
    assert res == {0: G.ERR_IO, 1: G.ERR_IO}
    assert os.listdir(tmp_path) == []
    # a published file left behind by an EARLIER job (same path, same size, valid magic, old
    # nonces, another id) is not taken for this job's id
    path = str(tmp_path / "c.id")
    old_id = bytes(128)
    rec = np.array([0x31305644524d4847, 3, 111, 222], dtype=np.uint64).tobytes() + old_id
    open(path, "wb").write(rec)
    res = _rdv_threads(G, path, 3, 10.0, ident, delays={0: 0.3})
    assert res == {0: ident, 1: ident, 2: ident}
    assert os.listdir(tmp_path) == []
    # a JOIN file left behind by a crashed rank 1 of an earlier job: rank 0 first publishes
    # with that stale nonce, the real rank 1 arrives later with a fresh one and is served
    path = str(tmp_path / "d.id")
    open(path + ".join.1", "wb").write(np.array([0x31305644524d4847, 1, 999], dtype=np.uint64).tobytes())
    res = _rdv_threads(G, path, 2, 10.0, ident, delays={1: 0.3})
    assert res == {0: ident, 1: ident}
    assert os.listdir(tmp_path) == []
    # bad arguments
    for args in (("", 0, 2), (path, 2, 2), (path, -1, 2), (path, 0, 0)):
        with pytest.raises(G.GhmmError) as e:
            G.rendezvous_file(args[0], args[1], args[2], 0.1, ident)
        assert e.value.code == G.ERR_ARG


def test_bench_dump_outputs(tmp_path):
    """bench.py --dump-outputs: one float64 .npy per array; above the size limit, the same seeded
    sample of every array in every run, within the limit (under 64 MB by default)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.DUMP_LIMIT_BYTES + 16 * 128 <= 64 * 10 ** 6     # the arrays and their .npy headers
    arrays = {"a": np.arange(1000.0).reshape(10, 100), "b": np.arange(3000, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    assert sorted(os.listdir(tmp_path / "all")) == ["a.npy", "b.npy"]
    for k, v in arrays.items():
        got = np.load(tmp_path / "all" / f"{k}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, v)
    runs = []
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=8000)
        runs.append({k: np.load(tmp_path / d / f"{k}.npy") for k in arrays})
    assert sum(a.nbytes for a in runs[0].values()) <= 8000
    for k, v in arrays.items():
        a = runs[0][k]
        assert a.size >= 200 and np.array_equal(a, runs[1][k])
        assert np.isin(a, v).all() and (np.diff(a) > 0).all()   # distinct entries, in storage order
