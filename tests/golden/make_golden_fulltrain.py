#!/usr/bin/env python3
"""Generates the full-covariance trainer's fixtures in this directory from the REAL reference.

Run in the build container only (needs the reference tree and gcc):
    python tests/golden/make_golden_fulltrain.py

The reference's full-covariance trainer (train/source/hmm-full-fs/hmm_continuous_full_fs.c,
"TFF") is compiled as shipped, without any edit (gcc -O2 -w -ffp-contract=off), into a temporary
directory that is deleted afterwards, and run with the stack limit raised and the reference's argv
(train/test/Run Arguments.txt):
    <word> <N> 1 <M> list.txt out.hmm
Recorded:
  (a) "shipped": the 13 runs of train/test/result, <word> 6 1 1 over a list holding the one bundled
      utterance of the word (perfil/).  Each report must equal the shipped
      train/test/result/*.txt apart from the file-name and time lines (so: the same mean
      probability and number of iterations), which is checked here.  The models are those of this
      64-bit build (the shipped .hmm, in full_cov_models/, come from a 32-bit one; they differ by
      at most ~1.5e-8 relative).
  (b) "synthetic", inside TFF's caps (D = 9, M <= 3, N <= 20, T <= 500): three words drawn from
      known full-covariance models, N x M = 5x2, 8x3 and 12x2, 6-10 utterances each.
      Checked here: every recorded det is non-zero, every score is finite, and no printed
      "Verifying Probability" lies within 1e-5 of the threshold (stable iteration counts).
      There is no word on which treat_zero_det (TFF:2226) fires: every variant tried (five or four
      near-constant coefficients, one state with a covariance scaled by 0.05 or 0.08) makes TFF's
      own run end in a NaN or -inf mean probability, so it is no usable golden.
      tests/test_fulltrain_host.py covers that function against a numpy restatement instead.
Outputs (data only; nothing of TFF and no binary is stored):
  fulltrain_runs.json      per run: argv shape, report lines (time lines dropped) and the printed
                           "Verifying Probability" values
  fulltrain_models.npz     the models every run wrote ("<run>.A/.c/.mean/.det/.inv_cov")
  fulltrain_synth.npz      the synthetic utterances ("<word>.X", float32-representable, and
                           "<word>.lens")
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
TFF = os.path.join(REF, "train/source/hmm-full-fs/hmm_continuous_full_fs.c")
RESULT = os.path.join(REF, "train/test/result")
SEED = 20261017
THRESHOLD = 1.0e-3
SKIP = ("starting time", "ending time", "cpu time")
# (word, N, M, utterances)
SYNTH = [("syn_a", 5, 2, 8), ("syn_b", 8, 3, 6), ("syn_c", 12, 2, 10)]
D_SYNTH = 9


def big_stack():
    resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))


def report_lines(txt):
    return [l for l in txt.split("\n") if l and not l.startswith(SKIP)]


def shipped_words():
    return sorted(f[len("mean_"):-len(".txt")] for f in os.listdir(RESULT) if f.endswith(".txt"))


def run_tff(exe, tmp, word, N, M, perfils):
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(perfils) + "\n")
    for fn in ("out.hmm", "out.txt"):
        if os.path.exists(os.path.join(tmp, fn)):
            os.remove(os.path.join(tmp, fn))
    p = subprocess.run([exe, word, str(N), "1", str(M), "list.txt", "out.hmm"], cwd=tmp,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, preexec_fn=big_stack)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-2000:]
    verify = [float(v) for v in re.findall(r"Verifying Probability: (\S+) >", out)]
    report = report_lines(open(os.path.join(tmp, "out.txt")).read())
    hm = G.HostFullModel.read(os.path.join(tmp, "out.hmm"))
    return report, verify, hm


def synth_word(rng, N, M, n_utt):
    """utterances of a random left-to-right full-covariance model: (X, lens)"""
    D = D_SYNTH
    mean = rng.normal(0.0, 2.0, (N, M, D))
    chol = []
    for _ in range(N * M):
        Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
        chol.append(np.linalg.cholesky((Q * rng.uniform(0.3, 1.5, D)) @ Q.T))
    c = np.stack([rng.dirichlet(np.full(M, 4.0)) for _ in range(N)])
    lens = [int(v) for v in rng.integers(max(60, 12 * N), 401, n_utt)]
    Xs = []
    for T in lens:
        cuts = np.sort(rng.choice(np.arange(1, T), N - 1, replace=False))
        state = np.searchsorted(cuts, np.arange(T), side="right")
        X = np.empty((T, D))
        for t in range(T):
            i = state[t]
            k = rng.choice(M, p=c[i])
            X[t] = mean[i, k] + chol[i * M + k] @ rng.normal(size=D)
        Xs.append(np.asarray(X, dtype=np.float32).astype(np.float64))
    return Xs, lens


def main():
    assert os.path.exists(TFF), "reference not present"
    runs, models, synth = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hmm-full")
        subprocess.check_call(["gcc", "-O2", "-w", "-ffp-contract=off", TFF, "-o", exe, "-lm"])

        # (a) the 13 shipped runs
        for word in shipped_words():
            fn = f"mean_{word}.perfil"
            shutil.copyfile(os.path.join(HERE, "perfil", fn), os.path.join(tmp, fn))
            report, verify, hm = run_tff(exe, tmp, word, 6, 1, [fn])
            shipped = report_lines(open(os.path.join(RESULT, f"mean_{word}.txt")).read())
            same = lambda ls: [l for l in ls if not l.startswith(("model file", "parameter 1"))]  # noqa: E731
            assert same(report) == same(shipped), f"TFF does not reproduce the shipped report of {word}"
            runs[word] = {"kind": "shipped", "N": 6, "M": 1, "perfils": [fn], "report": report,
                          "verify": verify}
            models[word] = hm
            print(word, report[-2:])

        # (b) synthetic
        rng = np.random.default_rng(SEED)
        for word, N, M, n_utt in SYNTH:
            Xs, lens = synth_word(rng, N, M, n_utt)
            names = []
            for u, X in enumerate(Xs):
                names.append(f"{word}_{u}.perfil")
                G.perfil_write(os.path.join(tmp, names[-1]), X)
            report, verify, hm = run_tff(exe, tmp, word, N, M, names)
            assert np.all(hm.det != 0.0), f"{word}: a recorded det is 0"
            prob = float(next(l for l in report if l.startswith("mean probability")).split(":")[1])
            assert np.isfinite(prob), f"{word}: score not finite"
            assert all(abs(v - THRESHOLD) > 1e-5 for v in verify), f"{word}: a variation near the threshold"
            runs[word] = {"kind": "synthetic", "N": N, "M": M, "perfils": names, "report": report,
                          "verify": verify}
            models[word] = hm
            synth[word + ".X"] = np.concatenate(Xs).astype(np.float32)
            synth[word + ".lens"] = np.array(lens, dtype=np.int32)
            print(word, report[-2:], "min det", hm.det.min())

    with open(os.path.join(HERE, "fulltrain_runs.json"), "w") as f:
        json.dump(runs, f, indent=1)
    arrays = {}
    for word, hm in models.items():
        for name in ("A", "c", "mean", "det", "inv_cov"):
            arrays[f"{word}.{name}"] = getattr(hm, name)
    np.savez_compressed(os.path.join(HERE, "fulltrain_models.npz"), **arrays)
    np.savez_compressed(os.path.join(HERE, "fulltrain_synth.npz"), **synth)
    print("done")


if __name__ == "__main__":
    main()
