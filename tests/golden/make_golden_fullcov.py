#!/usr/bin/env python3
"""Generates the full-covariance recogniser's fixtures in this directory from the REAL reference.

Run in the build container only (needs the reference tree and gcc):
    python tests/golden/make_golden_fullcov.py

The reference's full-covariance recogniser (test/source/recognition-full-fs/
recognition_continuous_full_fs.c, "RC") is compiled as shipped, without any edit
(gcc -O2 -w -ffp-contract=off), into a temporary directory that is deleted afterwards, and run
with the stack limit raised and the reference's argv (test/test/Run Arguments.txt):
    1 models.txt 1 mean_list.txt words.txt out.txt
Recorded:
  (a) "shipped": the 13 shipped models (full_cov_models/, rewritten with the 8-byte length prefix
      a 64-bit build reads) on the 13 bundled utterances (perfil/), lists in the reference's order;
      the report must equal the shipped test/test/result/hmm-result.txt line for line (date, CPU
      time and model-name lines aside), which is checked here.
  (b) "synthetic": 13 words x 12 states x 4 mixtures x 16 coefficients (inside RC's caps), random
      well-conditioned SPD inverse covariances from a fixed seed, one utterance of 80-400 frames
      per word drawn from its own model.  Every one of the 169 scores is finite.
Outputs (data only; nothing of RC and no binary is stored):
  fullcov_recog.json    stdout rankings ("<word> :  <score>", 13 rows per spoken word) and the
                        report of both runs
  fullcov_synth13.npz   the synthetic models and frames.  Values are float32-representable and
                        inv_cov is stored as its upper triangle (the matrices are symmetric), so
                        that the file stays small: inv_cov[j][i] = inv_cov[i][j] = iu[k] for the
                        k-th pair (i <= j) of numpy.triu_indices(16)
  fullcov_hmm_result.txt  the shipped hmm-result.txt, verbatim
"""
import json
import os
import re
import resource
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _load import ghmm as _ghmm  # noqa: E402

G = _ghmm()
REF = os.environ.get("GHMM_REFERENCE", "/root/reference")
RC = os.path.join(REF, "test/source/recognition-full-fs/recognition_continuous_full_fs.c")
WORDS = [l.strip() for l in open(os.path.join(REF, "test/test/words.txt")) if l.strip()]
MEAN_LIST = [os.path.basename(l.strip()) for l in
             open(os.path.join(REF, "test/test/perfil_data/mean_list.txt")) if l.strip()]
MODEL_LIST = [os.path.basename(l.strip()) for l in
              open(os.path.join(REF, "test/test/models/models.txt")) if l.strip()]
SKIP = ("Date and time", "Model name")
SEED = 20261016


def big_stack():
    resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))


def report_lines(txt):
    return [l for l in txt.split("\n") if not l.startswith(SKIP) and "recognition time" not in l]


def parse_stdout(out):
    blocks, cur = [], None
    for line in out.replace("\r", "").split("\n"):
        m = re.match(r"Spoken word: (\S+)", line)
        if m:
            cur = {"spoken": m.group(1), "ranking": []}
            blocks.append(cur)
            continue
        m = re.match(r"(\S+) :  (\S+) $", line)
        if m and cur is not None:
            cur["ranking"].append([m.group(1), m.group(2)])
    return blocks


def run_rc(exe, tmp, models, perfils, words):
    """models / perfils: file names inside tmp (RC keeps names in 100-byte buffers)"""
    for name, lines in (("models.txt", models), ("mean_list.txt", perfils), ("words.txt", words)):
        with open(os.path.join(tmp, name), "w") as f:
            f.write("\n".join(lines) + "\n")
    p = subprocess.run([exe, "1", "models.txt", "1", "mean_list.txt", "words.txt", "out.txt"], cwd=tmp,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, preexec_fn=big_stack)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-2000:]
    return parse_stdout(out), report_lines(open(os.path.join(tmp, "out.txt")).read())


def synth_models(rng, n_words=13, N=12, M=4, D=16):
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # noqa: E731
    base = rng.normal(0.0, 2.0, (N, M, D))
    iu = np.triu_indices(D)
    words, models, tri = [], [], []
    for w in range(n_words):
        A = np.zeros((N, N))
        for i in range(N - 1):
            A[i, i] = f32(rng.uniform(0.6, 0.9))
            A[i, i + 1] = 1.0 - A[i, i]
        A[N - 1, N - 1] = 1.0
        c = np.stack([f32(rng.dirichlet(np.full(M, 4.0))) for _ in range(N)])
        mean = f32(base + rng.normal(0.0, 0.4, (N, M, D)))
        ic = np.empty((N, M, D, D))
        t = np.empty((N, M, len(iu[0])))
        for i in range(N):
            for k in range(M):
                Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
                S = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
                u = f32(S[iu])
                S = np.zeros((D, D))
                S[iu] = u
                S = S + np.triu(S, 1).T
                ic[i, k], t[i, k] = S, u
        det = 1.0 / np.linalg.det(ic)  # of the NON-inverted covariance, as the .hmm file holds it
        words.append(f"syn{w:02d}")
        models.append(G.HostFullModel(A, c, mean, ic, det, word=words[-1]))
        tri.append(t)
    return words, models, tri


def synth_utterance(rng, hm, T):
    """left-to-right walk through the states (about T / N frames each), one mixture per frame"""
    N, M, D = hm.N, hm.M, hm.D
    cuts = np.sort(rng.choice(np.arange(1, T), N - 1, replace=False))
    state = np.searchsorted(cuts, np.arange(T), side="right")
    X = np.empty((T, D))
    for t in range(T):
        i = state[t]
        k = rng.choice(M, p=hm.c[i] / hm.c[i].sum())
        cov = np.linalg.inv(hm.inv_cov[i, k])
        X[t] = rng.multivariate_normal(hm.mean[i, k], (cov + cov.T) / 2)
    return np.asarray(X, dtype=np.float32).astype(np.float64)


def main():
    assert os.path.exists(RC), "reference not present"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "recognition-full")
        subprocess.check_call(["gcc", "-O2", "-w", "-ffp-contract=off", RC, "-o", exe, "-lm"])

        # (a) the shipped models and utterances
        with tempfile.TemporaryDirectory() as run:
            for fn in MODEL_LIST:
                G.HostFullModel.read(os.path.join(HERE, "full_cov_models", fn)).write(os.path.join(run, fn), 8)
            for fn in MEAN_LIST:
                shutil.copyfile(os.path.join(HERE, "perfil", fn), os.path.join(run, fn))
            blocks, report = run_rc(exe, run, MODEL_LIST, MEAN_LIST, WORDS)
        shipped = open(os.path.join(REF, "test/test/result/hmm-result.txt")).read()
        assert report == report_lines(shipped), "RC does not reproduce the shipped hmm-result.txt"
        shutil.copyfile(os.path.join(REF, "test/test/result/hmm-result.txt"),
                        os.path.join(HERE, "fullcov_hmm_result.txt"))
        out["shipped"] = {"words": WORDS, "models": MODEL_LIST, "mean_list": MEAN_LIST,
                          "blocks": blocks, "report": report}
        print("shipped:", report[-6:])

        # (b) synthetic, every score finite
        rng = np.random.default_rng(SEED)
        words, models, tri = synth_models(rng)
        lens = [int(v) for v in rng.integers(80, 401, len(words))]
        Xs = [synth_utterance(rng, hm, T) for hm, T in zip(models, lens)]
        with tempfile.TemporaryDirectory() as run:
            mnames, pnames = [], []
            for w, hm, X in zip(words, models, Xs):
                hm.write(os.path.join(run, w + ".hmm"), 8)
                G.perfil_write(os.path.join(run, w + ".perfil"), X)
                mnames.append(w + ".hmm")
                pnames.append(w + ".perfil")
            blocks, report = run_rc(exe, run, mnames, pnames, words)
        vals = [float(v) for b in blocks for _, v in b["ranking"]]
        assert len(vals) == 169 and np.isfinite(vals).all(), "a synthetic score is not finite"
        out["synthetic"] = {"words": words, "lens": lens, "blocks": blocks, "report": report}
        arrays = {"lens": np.array(lens, dtype=np.int32)}
        for w, hm, t, X in zip(words, models, tri, Xs):
            arrays[w + ".A"] = hm.A
            arrays[w + ".c"] = hm.c.astype(np.float32)
            arrays[w + ".mean"] = hm.mean.astype(np.float32)
            arrays[w + ".inv_cov_triu"] = t.astype(np.float32)
            arrays[w + ".det"] = hm.det
            arrays[w + ".X"] = X.astype(np.float32)
        np.savez_compressed(os.path.join(HERE, "fullcov_synth13.npz"), **arrays)
        print("synthetic:", report[-6:])
    with open(os.path.join(HERE, "fullcov_recog.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("done")


if __name__ == "__main__":
    main()
