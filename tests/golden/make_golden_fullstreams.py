#!/usr/bin/env python3
"""Generates the fixtures of the full-covariance programs on several feature streams (param_number
= 2) in this directory from the REAL reference.

Run in the build container only (needs the reference tree and gcc):
    python tests/golden/make_golden_fullstreams.py

The reference's full-covariance trainer (train/source/hmm-full-fs/hmm_continuous_full_fs.c, "TFF")
and recogniser (test/source/recognition-full-fs/recognition_continuous_full_fs.c, "RC") are compiled
as shipped, without any edit (gcc -O2 -w -ffp-contract=off), into a temporary directory that is
deleted afterwards, and run there with the stack limit raised.  Stream 1 is the bundled 9-d frames
(perfil/), stream 2 tests/streams_util.second_stream of them (5-d), as in make_golden_streams.py.
Recorded, all inside the programs' shipped caps (D <= 9, M <= 3, N <= 20, T <= 500):
  "train"        three runs over all 13 bundled utterances, argv
                     <name> <N> 2 <M1> <M2> list1.txt list2.txt <name>.hmm
                 with (N, M1, M2) = (6, 2, 1), (4, 2, 2), (5, 1, 1)
  "word_models"  thirteen one-utterance word models, argv  <word> 6 2 1 1 l1.txt l2.txt <word>.hmm
  "recog"        RC on those thirteen models and the 13 utterances, argv
                     1 models.txt 1 list1.txt list2.txt words.txt report.txt
Checked here: every recorded det is non-zero, every mean probability is finite, and no printed
"Verifying Probability" lies within 1e-5 of the 1e-3 threshold (stable iteration counts).
Outputs (data only; nothing of TFF or RC and no binary is stored):
  fullstreams_p2.json      per training run: argv shape, report lines (time lines dropped) and every
                           printed "Verifying Probability"; RC's printed ranking blocks and report lines
  fullstreams_models.npz   every written model, parsed by read_fhmm_streams below:
                           "<run>.A", "<run>.s<p>.c / .mean / .det / .inv_cov"
  full_streams_models/all13_6_p2.hmm   the file TFF itself wrote for the 6-state run (a reader fixture)
"""
import json
import os
import re
import resource
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _load import ghmm as _ghmm  # noqa: E402
from streams_util import second_stream  # noqa: E402

G = _ghmm()
REF = os.environ.get("GHMM_REFERENCE", "/root/reference")
TFF = os.path.join(REF, "train/source/hmm-full-fs/hmm_continuous_full_fs.c")
RC = os.path.join(REF, "test/source/recognition-full-fs/recognition_continuous_full_fs.c")
WORDS = [l.strip() for l in open(os.path.join(REF, "test/test/words.txt")) if l.strip()]
MEAN_LIST = [os.path.basename(l.strip()) for l in
             open(os.path.join(REF, "test/test/perfil_data/mean_list.txt")) if l.strip()]
THRESHOLD = 1.0e-3
SKIP = ("starting time", "ending time", "cpu time")
# (run, N, [M1, M2]) over all 13 utterances
TRAIN = [("all13_6_p2", 6, [2, 1]), ("all13_4_p2", 4, [2, 2]), ("all13_5_p2", 5, [1, 1])]
FIXTURE = "all13_6_p2"


def big_stack():
    resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))


def read_fhmm_streams(path):
    """Parser of the reference's full-covariance .hmm layout for P streams (TFF:2278-2400), 8-byte
    length prefix: (word, A, [per stream a dict of c, mean, det, inv_cov])"""
    raw = open(path, "rb").read()
    o = 0
    (n,) = struct.unpack_from("<Q", raw, o); o += 8
    word = raw[o:o + n].decode(); o += n
    N, P = struct.unpack_from("<ii", raw, o); o += 8
    M = list(struct.unpack_from(f"<{P}i", raw, o)); o += 4 * P
    D = list(struct.unpack_from(f"<{P}i", raw, o)); o += 4 * P
    A = np.frombuffer(raw, "<f8", N * N, o).reshape(N, N).copy(); o += 8 * N * N
    streams = []
    for p in range(P):
        c = np.zeros((N, M[p])); mean = np.zeros((N, M[p], D[p])); det = np.zeros((N, M[p]))
        ic = np.zeros((N, M[p], D[p], D[p]))
        for i in range(N):
            c[i] = np.frombuffer(raw, "<f8", M[p], o); o += 8 * M[p]
            for k in range(M[p]):
                mean[i, k] = np.frombuffer(raw, "<f8", D[p], o); o += 8 * D[p]
                (det[i, k],) = struct.unpack_from("<d", raw, o); o += 8
                ic[i, k] = np.frombuffer(raw, "<f8", D[p] * D[p], o).reshape(D[p], D[p]); o += 8 * D[p] * D[p]
        streams.append({"c": c, "mean": mean, "det": det, "inv_cov": ic})
    assert o == len(raw), (o, len(raw))
    return word, A, streams


def report_lines(txt):
    return [l for l in txt.split("\n") if l and not l.startswith(SKIP)]


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


def write_lists(tmp, tag, idx):
    """file names inside tmp (the programs keep names in 100-byte buffers)"""
    names = []
    for s, prefix in ((1, ""), (2, "d_")):
        names.append(f"{tag}_{s}.txt")
        with open(os.path.join(tmp, names[-1]), "w") as f:
            f.write("\n".join(prefix + MEAN_LIST[i] for i in idx) + "\n")
    return names


def run_tff(exe, tmp, name, N, Ms, idx):
    lists = write_lists(tmp, name, idx)
    argv = [name, str(N), str(len(Ms))] + [str(m) for m in Ms] + lists + [name + ".hmm"]
    p = subprocess.run([exe] + argv, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       preexec_fn=big_stack)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-2000:]
    verify = [float(v) for v in re.findall(r"Verifying Probability: (\S+) >", out)]
    report = report_lines(open(os.path.join(tmp, name + ".txt")).read())
    word, A, streams = read_fhmm_streams(os.path.join(tmp, name + ".hmm"))
    assert word == name
    for p_, s in enumerate(streams):
        assert np.all(s["det"] != 0.0), f"{name}: a recorded det of stream {p_ + 1} is 0"
    prob = float(next(l for l in report if l.startswith("mean probability")).split(":")[1])
    assert np.isfinite(prob), f"{name}: mean probability not finite"
    assert all(abs(v - THRESHOLD) > 1e-5 for v in verify), f"{name}: a variation near the threshold: {verify}"
    run = {"N": N, "M": Ms, "utterances": list(idx),
           "argv": ["<word>", "N", "P"] + [f"M{k + 1}" for k in range(len(Ms))] +
                   [f"list{k + 1}" for k in range(len(Ms))] + ["<word>.hmm"],
           "report": report, "verify": verify}
    return run, A, streams


def main():
    assert os.path.exists(TFF) and os.path.exists(RC), "reference not present"
    out = {"words": WORDS, "mean_list": MEAN_LIST, "D2": 5, "train": {}, "word_models": {}}
    arrays = {}

    def keep(name, A, streams):
        arrays[f"{name}.A"] = A
        for p, s in enumerate(streams):
            for key, v in s.items():
                arrays[f"{name}.s{p}.{key}"] = v

    with tempfile.TemporaryDirectory() as tmp:
        tff, rc_exe = os.path.join(tmp, "tff"), os.path.join(tmp, "rc")
        for src, exe in ((TFF, tff), (RC, rc_exe)):
            subprocess.check_call(["gcc", "-O2", "-w", "-ffp-contract=off", src, "-o", exe, "-lm"])
        for fn in MEAN_LIST:
            shutil.copyfile(os.path.join(HERE, "perfil", fn), os.path.join(tmp, fn))
            G.perfil_write(os.path.join(tmp, "d_" + fn), second_stream(G.perfil_read(os.path.join(tmp, fn))))

        for name, N, Ms in TRAIN:
            run, A, streams = run_tff(tff, tmp, name, N, Ms, range(13))
            out["train"][name] = run
            keep(name, A, streams)
            print(name, run["report"][-2:], run["verify"][-3:])
        os.makedirs(os.path.join(HERE, "full_streams_models"), exist_ok=True)
        shutil.copyfile(os.path.join(tmp, FIXTURE + ".hmm"),
                        os.path.join(HERE, "full_streams_models", FIXTURE + ".hmm"))

        # one model per word from its own utterance, then the recogniser over all 13 utterances
        by_word = {fn[len("mean_"):-len(".perfil")]: k for k, fn in enumerate(MEAN_LIST)}
        for w in WORDS:
            run, A, streams = run_tff(tff, tmp, w, 6, [1, 1], [by_word[w]])
            out["word_models"][w] = run
            keep(w, A, streams)
            print(w, run["report"][-2:])
        lists = write_lists(tmp, "rec", range(13))
        for fn, lines in (("models.txt", [w + ".hmm" for w in WORDS]), ("words.txt", WORDS)):
            with open(os.path.join(tmp, fn), "w") as f:
                f.write("\n".join(lines) + "\n")
        p = subprocess.run([rc_exe, "1", "models.txt", "1"] + lists + ["words.txt", "report.txt"], cwd=tmp,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, preexec_fn=big_stack)
        txt = p.stdout.decode(errors="replace")
        assert p.returncode == 0, txt[-2000:]
        report = open(os.path.join(tmp, "report.txt")).read()
    blocks = parse_stdout(txt)
    assert len(blocks) == 13 and all(len(b["ranking"]) == 13 for b in blocks)
    out["recog"] = {"argv": ["1", "models.txt", "1", "list1", "list2", "words.txt", "report.txt"],
                    "blocks": blocks,
                    "report": [l for l in report.split("\n") if not l.startswith(("Date and time", "Model name"))
                               and "recognition time" not in l]}
    with open(os.path.join(HERE, "fullstreams_p2.json"), "w") as f:
        json.dump(out, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "fullstreams_models.npz"), **arrays)
    print("done:", len(blocks), "recognition blocks")


if __name__ == "__main__":
    main()
