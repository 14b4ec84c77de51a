"""The two recognisers' command lines with GHMM_CONFIDENCE=1 beside GHMM_CONNECTED=1 — GPU box only: every
decoded word printed with its confidence, the line closed by the Viterbi score and log P, equal to
word_confidence of the Python path to the two printed digits; without the variable the output is the
connected-word decoder's as it was.  (The two exit-1 refusals are test_gpost_host.py's: they need no GPU.)"""
import os
import subprocess

import numpy as np
import pytest

import connect_cases as CC
import grammar_cases as GC
from _load import PKG_DIR
from fullcov_support import ctx  # noqa: F401  (the fixture)
from fullcov_support import fmt, offsets
from test_grammar_gpu import write_files, write_grammar

pytestmark = pytest.mark.gpu

BIN = {False: os.path.join(PKG_DIR, "bin", "recognition-continuous-test-fs"),
       True: os.path.join(PKG_DIR, "bin", "recognition-continuous-test-full-fs")}
OURS = ("GHMM_CONNECTED", "GHMM_WORD_PENALTY", "GHMM_GRAMMAR", "GHMM_ALIGN", "GHMM_CONFIDENCE")


def run(binary, tmp, args, env):
    e = {k: v for k, v in os.environ.items() if k not in OURS}
    e.update(env)
    p = subprocess.run([binary] + args, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=e)
    return p.returncode, p.stdout.decode(errors="replace")


class Files:
    """what test_grammar_gpu.write_files reads of a device: the case and its model kind"""

    def __init__(self, case, full):
        self.case, self.full = case, full


@pytest.mark.parametrize("name", ["mixed", "full"])
def test_command_line_with_confidences(G, ctx, tmp_path, name):
    case = GC.make(G, name)
    full = name in GC.FULLCOV
    d = Files(case, full)
    tmp = str(tmp_path)
    utts, lists, names = write_files(G, tmp, d)
    off = offsets(case.lens)
    args = ["1", "models.txt", "1"] + lists + ["words.txt", "report.txt"]
    HM = G.HostFullModel if full else G.HostModel
    mk = ctx.full_model if full else ctx.model
    dms = [[mk(h) for h in HM.read_streams(os.path.join(tmp, w + ".hmm"))] for w in names]
    lens = case.lens[utts]
    corpora = [ctx.corpus(np.concatenate([X[off[u]:off[u + 1]] for u in utts]), lens) for X in case.Xs]
    start, pair, fin = GC.random(case.K, GC.RANDOM_SEED[name])
    write_grammar(os.path.join(tmp, "g.txt"), start, pair, fin)
    connect = ctx.connect_full_streams if full else ctx.connect_streams
    grammar = ctx.connect_grammar_full_streams if full else ctx.connect_grammar_streams
    post = ctx.grammar_post_full_streams if full else ctx.grammar_post_streams

    def lines(word, begin, score, occ=None, ll=None):
        seg = G.word_segments(word, begin, lens)
        if occ is None:
            return [f"s0_u{u}.perfil : " + "".join(names[k] + " " for k, _, _ in s) + ": " + fmt(sc)
                    for u, s, sc in zip(utts, seg, score)]
        conf = G.word_confidence(seg, occ, lens)
        return [f"s0_u{u}.perfil : " + "".join(f"{names[k]}({c:.2f}) " for k, _, _, c in s) + ": " + fmt(sc) + " " + fmt(l)
                for u, s, sc, l in zip(utts, conf, score, ll)]
    try:
        # under the grammar file (the penalty added to every pair score), and without one: the flat grammar
        for env, decode, g in (
                ({"GHMM_GRAMMAR": "g.txt", "GHMM_WORD_PENALTY": "-1.5"},
                 lambda: grammar(dms, corpora, pair - 1.5, start, fin), (start, pair - 1.5, fin)),
                ({"GHMM_WORD_PENALTY": "-5"}, lambda: connect(dms, corpora, -5.0), GC.flat(case.K, -5.0))):
            word, path, begin, score = decode()
            occ, ll = post(dms, corpora, g[1], g[0], g[2])
            want = lines(word, begin, score, occ, ll)
            assert any("(" in l for l in want)
            rc, text = run(BIN[full], tmp, args, dict(env, GHMM_CONNECTED="1", GHMM_CONFIDENCE="1"))
            assert rc == 0, text[-2000:]
            assert [l for l in text.replace("\r", "").split("\n") if l.startswith("s0_u")] == want
            rep = open(os.path.join(tmp, "report.txt")).read().split("\n")
            assert "Connected word recognition" in rep[0] and "confidences" in rep[0]
            assert ("grammar g.txt" in rep[0]) == ("GHMM_GRAMMAR" in env)
            assert rep[1:1 + len(want)] == want and rep[1 + len(want):] == [""]
            # without the variable: the decoder's lines and first line as they were
            plain = lines(word, begin, score)
            rc, text = run(BIN[full], tmp, args, dict(env, GHMM_CONNECTED="1"))
            assert rc == 0, text[-2000:]
            assert [l for l in text.replace("\r", "").split("\n") if l.startswith("s0_u")] == plain
            rep = open(os.path.join(tmp, "report.txt")).read().split("\n")
            p = float(env["GHMM_WORD_PENALTY"])
            assert rep[0].endswith(f"word penalty {p:g}, grammar g.txt " if "GHMM_GRAMMAR" in env else f"word penalty {p:g} ")
            assert "confidences" not in rep[0] and rep[1:1 + len(plain)] == plain and rep[1 + len(plain):] == [""]
    finally:
        for o in [m for w in dms for m in w] + corpora:
            o.close()
