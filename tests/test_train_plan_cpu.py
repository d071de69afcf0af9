"""The route of a training's begin (csrc/train_plan.h: plan_begin) and the sizing arithmetic of the 32-bit loop's pair
table (table_bits, wide_headroom), without a GPU: tests/train_plan_check.cpp answers requests on standard input, built
by the host compiler once plain and once under ASan + UBSan (stand-alone: nothing is loaded into Python).

plan_begin is asked every combination of the corpus' kind, the options and the request listed below and compared --
return code, route, the slot stream's vocab_size, the barrier layout -- with model(), which is written from the rules
of include/mbpe.h: the comments on mbpe_train_begin and mbpe_train_begin_from, on the options "chunk_barrier",
"wide_from", "first_wide", "resume_wide", "min_frequency" / "max_token_length", on the weighted loads, and the order
in which the entry points always gave simultaneous refusals.  The model does not read the header under test."""
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")
INCLUDE = os.path.join(HERE, "..", "include")

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}

OK, ERR_VOCAB, ERR_STATE = 0, -4, -5                                  # mbpe.h: mbpe_status
MAX_BASIC, MAX_ENDBIT, MAX_CHUNKED, MAX_WIDE = 65534, 32766, 65518, 1 << 24
SLOT, SLOT_THEN_WIDE, WIDE_DIRECT = 0, 1, 2

VOCABS = [256, 257, 32766, 32767, 65518, 65519, 65534, 65535, 1 << 24, (1 << 24) + 1]
WIDE_FROMS = [-1, 0, 5, 100000]


@pytest.fixture(scope="module", params=sorted(FLAGS))
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("train_plan_check_" + request.param) / "train_plan_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] +
                          FLAGS[request.param] + ["-I" + CSRC, "-I" + INCLUDE, os.path.join(HERE, "train_plan_check.cpp"),
                                                  "-o", path])
    return path


def ask(exe, requests):
    r = subprocess.run([exe], input="".join(line + "\n" for line in requests), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr.strip().endswith("%d requests" % len(requests))
    answers = r.stdout.split("\n")[:-1]
    assert len(answers) == len(requests)
    return answers


def slot_limit(chunked, chunk_barrier):
    """vmax: the largest vocab_size the 16-bit slot stream of this corpus holds."""
    if not chunked:
        return MAX_BASIC
    return MAX_ENDBIT if chunk_barrier == 0 else MAX_CHUNKED


def handover(chunked, chunk_barrier, wide_from):
    """h: the merge at which the slot stream hands over."""
    h = slot_limit(chunked, chunk_barrier) - 256
    return min(wide_from, h) if wide_from >= 0 else h


def model(chunked, chunk_barrier, first, first_wide, resume_wide, wide_from, weighted, limited, multi, vocab, n_prior):
    """-> (rc, route, slot_vocab, barrier); route and slot_vocab None where they say nothing (a refusal; no slot stream)."""
    vmax, T = slot_limit(chunked, chunk_barrier), vocab - 256
    barrier = bool(chunked) and (chunk_barrier == 1 or (chunk_barrier == -1 and vocab > MAX_ENDBIT))
    refuse = lambda rc: (rc, None, None, barrier)
    if weighted or limited:                  # 32-bit tokens from the first new merge, whatever else is set; one rank
        if multi:
            return refuse(ERR_STATE)
        if vocab > MAX_WIDE:
            return refuse(ERR_VOCAB)
        return OK, WIDE_DIRECT, None, barrier
    if n_prior == 0:                         # mbpe_train_begin
        if vocab <= vmax and not (wide_from >= 0 and T > wide_from):
            return OK, SLOT, vocab, barrier
        if vocab > MAX_WIDE:
            return refuse(ERR_VOCAB)
        if (first and not first_wide) or multi:
            return refuse(ERR_VOCAB)
        return OK, SLOT_THEN_WIDE, (min(256 + wide_from, vmax) if wide_from >= 0 else vmax), barrier
    if multi:                                # mbpe_train_begin_from
        return refuse(ERR_STATE)
    h = handover(chunked, chunk_barrier, wide_from)
    if resume_wide and T > h:
        if vocab > MAX_WIDE:
            return refuse(ERR_VOCAB)
        if first and not first_wide:
            return refuse(ERR_VOCAB)
        if n_prior >= h:
            return OK, WIDE_DIRECT, None, barrier                  # the direct case
        return OK, SLOT_THEN_WIDE, 256 + h, barrier                # the mixed case
    if not resume_wide and (vocab > vmax or wide_from >= 0):
        return refuse(ERR_VOCAB)
    return OK, SLOT, vocab, barrier                                # the slot case


def cases():
    out = []
    for chunked, chunk_barrier, wide_from, vocab in itertools.product((0, 1), (-1, 0, 1), WIDE_FROMS, VOCABS):
        T, h = vocab - 256, handover(chunked, chunk_barrier, wide_from)
        priors = sorted({n for n in (0, 1, h - 1, h, h + 1, T) if 0 <= n <= T})
        for flags in itertools.product((0, 1), repeat=6):
            first, first_wide, resume_wide, weighted, limited, multi = flags
            for n_prior in priors:
                out.append((chunked, chunk_barrier, first, first_wide, resume_wide, wide_from, weighted, limited, multi,
                            vocab, n_prior))
    return out


def test_the_cases_reach_every_route_and_refusal():
    seen = {model(*c)[:2] for c in cases()}
    assert seen == {(OK, SLOT), (OK, SLOT_THEN_WIDE), (OK, WIDE_DIRECT), (ERR_VOCAB, None), (ERR_STATE, None)}
    # ... the mixed and the direct case of a continued training among them, and a handover below the format's limit
    assert any(model(*c)[1] == SLOT_THEN_WIDE and c[10] > 0 for c in cases())
    assert any(model(*c)[1] == WIDE_DIRECT and c[10] > 0 and not (c[6] or c[7]) for c in cases())
    assert any(model(*c)[1] == SLOT_THEN_WIDE and model(*c)[2] == 256 + 5 for c in cases())


def test_plan_begin_against_the_model(exe):
    cs = cases()
    answers = ask(exe, ["P " + " ".join(str(x) for x in c) for c in cs])
    bad = []
    for c, line in zip(cs, answers):
        fields, message = line.split("\t")
        rc, route, slot_vocab, barrier = (int(x) for x in fields.split())
        want = model(*c)
        ok = rc == want[0] and bool(barrier) == want[3] and (message == "") == (rc == OK)
        if want[1] is not None:
            ok = ok and route == want[1]
        if want[2] is not None:
            ok = ok and slot_vocab == want[2]
        if want[0] != OK:                    # every refusal of a continued training names its entry point, as ever
            ok = ok and (message.startswith("mbpe_train_begin_from: ") == (c[10] > 0 and not (c[6] or c[7]) and
                                                                            "vocab_size exceeds 16777216" not in message))
        if not ok:
            bad.append((c, line, want))
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(cs), bad[:3])


def test_table_bits(exe):
    entries = sorted({0, 1, 2047, 2048, 2049, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 1 << 31, 1 << 40} |
                     {(1 << k) + d for k in range(10, 31) for d in (-1, 0, 1)})
    for e, line in zip(entries, ask(exe, ["B %d" % e for e in entries])):
        ok, bits = (int(x) for x in line.split())
        fitting = [b for b in range(12, 32) if (1 << b) >= 2 * e]
        assert ok == (1 if fitting else 0), e
        assert ok == (1 if e <= 1 << 30 else 0), e
        if fitting:
            assert bits == fitting[0], e


def test_wide_headroom(exe):
    asks = [(top, pos, m) for top, pos in ((10 ** 9, 10), (5, 10 ** 9), (0, 7), (7, 0), ((1 << 31) - 1, 1 << 40))
            for m in (0, 1, 16)]
    for (top, pos, m), line in zip(asks, ask(exe, ["H %d %d %d" % a for a in asks])):
        assert int(line) == m * (2 * min(top, pos) + 2), (top, pos, m)
    assert (10 ** 9, 10, 16) in asks and any(m == 0 for _, _, m in asks)
