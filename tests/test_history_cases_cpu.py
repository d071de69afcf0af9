"""CPU tests of tests/history_cases.py: the schedules are what they claim to be, the composed references are more than
one implementation held against itself, and check() notices state that leaks from one call into the next -- shown with
a stand-in encoder in Python that answers from expected(step) and carries one stale-state defect at a time.  That is the
evidence that tests/test_gpu_encoder_history.py would catch such a defect in the library; no device code is touched."""
import collections

import numpy as np
import pytest

import byteoff_cases as B
import dropout_cases as D
import encode_rank_cases as R
import history_cases as HC
import oracle as O

HAND = [f.__name__ for f in HC.HAND_MADE]


def is_large(name):
    return name in ("large", "ones")


# ---- the schedules ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", HC.SEEDS)
def test_constructed_schedules_hold_their_conditions(seed):
    steps = HC.constructed(seed).steps
    classes = [s.route for s in steps]
    # 64 transitions, every ordered pair of classes exactly once, self-loops included
    pairs = collections.Counter(zip(classes[:-1], classes[1:]))
    assert len(steps) == 65 and len(pairs) == 64 and set(pairs.values()) == {1}
    assert set(pairs) == {(a, b) for a in HC.ROUTES for b in HC.ROUTES}
    # (a) every class: large before its first small call, and large again after its last small one
    for c in HC.ROUTES:
        sizes = [s.inp for s in steps if s.route == c]
        small = [k for k, n in enumerate(sizes) if n in HC.SMALL]
        assert small, c
        assert any(is_large(n) for n in sizes[:small[0]]), c
        assert any(is_large(n) for n in sizes[small[-1] + 1:]), c
    # (b) every setting is on, then off, then on again, each for at least one call that it reaches
    for name, (off, on) in HC.TOGGLES.items():
        reached = [s for s in steps if name != "count_ids" or s.route == "count"]
        values = [s.set[name] for s in reached]
        runs = [v for k, v in enumerate(values) if k == 0 or v != values[k - 1]]
        assert all(v in (off, on) for v in values) and off in values and on in values, name
        assert any(runs[k:k + 3] == [on, off, on] for k in range(len(runs))), (name, runs)
    # another seed, another schedule
    others = [HC.constructed(s) for s in HC.SEEDS if s != seed]
    assert all([s.route for s in o.steps] != classes for o in others)


def test_count_ids_changes_only_with_a_reset():
    for sched in HC.all_schedules():
        cur = 0
        for s in sched.steps:
            if s.route == "count":
                assert s.reset or s.set["count_ids"] == cur, (sched.name, s.describe())
                cur = s.set["count_ids"]


def test_hand_made_schedules_are_named_and_go_large_small_large():
    assert len(HC.HAND_MADE) == 8 and len(set(HAND)) == 8
    for name in HAND:
        sched = HC.hand_made(name)
        assert sched.name == name and sched.doc and "\n" not in sched.doc.strip()
        sizes = [HC.pool()[s.inp] for s in sched.steps]
        big = [k for k, i in enumerate(sizes) if len(i.data) > 2900]
        little = [k for k, i in enumerate(sizes) if i.name in HC.SMALL]
        if name != "widths_and_sides":                             # (that one keeps the size and turns the output)
            assert big and little and big[0] < little[0] < big[-1], name


def test_every_documented_refusal_is_a_step():
    """The nine refusals, each at least once over the schedules, each with its code."""
    seen = collections.Counter()
    for sched in HC.all_schedules():
        for s in sched.steps:
            code = HC.refusal(s)
            if code is None:
                assert HC.expected(s)["error"] == HC.OK
                continue
            assert HC.expected(s)["error"] == code
            t, st = HC._threshold(s), s.set
            why = ("dropout, greedy" if t and st["order"] == "greedy" else
                   "dropout, dedup" if t and st["dedup"] else
                   "byte_off, dedup" if s.byteoff and st["dedup"] and s.cap != "query" else
                   "fim and mlm" if s.route in HC.BATCH and st["fim"] and st["mlm"] else
                   "whole word, 16 bits" if s.route in HC.BATCH and st["mlm"] and st["mlm"]["whole_word"] and s.bits == 16 else
                   "single, 16 bits" if code == HC.ERR_VOCAB else
                   "chunk above piece_bytes" if code == HC.ERR_OOM and not s.endmask else
                   "endmask text above piece_bytes" if code == HC.ERR_OOM else "cap")
            seen[(why, code)] += 1
    want = {("dropout, greedy", HC.ERR_ARG), ("dropout, dedup", HC.ERR_ARG), ("byte_off, dedup", HC.ERR_ARG),
            ("fim and mlm", HC.ERR_ARG), ("whole word, 16 bits", HC.ERR_ARG), ("single, 16 bits", HC.ERR_VOCAB),
            ("cap", HC.ERR_ARG), ("chunk above piece_bytes", HC.ERR_OOM), ("endmask text above piece_bytes", HC.ERR_OOM)}
    assert set(seen) == want, sorted(set(seen) ^ want)
    # ... and most steps are calls that succeed
    n = sum(len(s.steps) for s in HC.all_schedules())
    assert sum(seen.values()) < n // 2


def test_steps_vary_what_the_issue_lists():
    steps = [s for sched in HC.all_schedules() for s in sched.steps]
    for field, values in (("text", {"host", "dev", "dev1"}), ("out", {"host", "dev"}), ("bits", {16, 32}),
                          ("cap", {"n", "query", "short"}), ("offsets", {False, True}), ("endmask", {False, True})):
        assert {getattr(s, field) for s in steps} == values, field
    for route in HC.ROUTES:
        forms = {(s.endmask, s.out) for s in steps if s.route == route}
        assert len(forms) >= (4 if route in HC.BATCH else 2), route
    flat = [s for s in steps if s.route == "endmask"]
    assert {bool(HC._singles_key(s)) for s in flat} == {False, True} and {s.docs for s in flat} == {False, True}
    assert {s.byteoff for s in flat} == {False, True}


# ---- the pool -------------------------------------------------------------------------------------------------------------

def _counts(name):
    inp = HC.pool()[name]
    lens = np.diff(inp.chunk_off.astype(np.int64))
    return dict(bytes=len(inp.data), chunks=int((lens > 0).sum()), docs=inp.n_docs, singles=len(HC.nul_singles(name)),
                tokens=min(len(HC.stream(name, o, None, "nul")[0]) for o in ("greedy", "rank")))


def test_the_pool_holds_what_the_schedules_are_for():
    large, medium = HC.pool()["large"], HC.pool()["medium"]
    L, Mc = _counts("large"), _counts("medium")
    assert 35000 <= L["bytes"] <= 45000 and 2500 <= Mc["bytes"] <= 3500
    assert L["chunks"] > 2049 and L["docs"] >= 1025 and L["singles"] > 256 and L["tokens"] > 2048
    for k in ("chunks", "docs", "singles", "tokens"):
        assert Mc[k] < L[k], k
    lens = np.diff(large.chunk_off.astype(np.int64))
    ones = "".join("1" if v == 1 else "0" for v in lens)
    assert "1" * 1100 in ones                                       # a span of the expansion that is full of ends
    assert lens[0] == 0 and lens[-1] == 0 and "000" in "".join("0" if v == 0 else "x" for v in lens)
    docs = np.diff(large.doc_chunk_off.astype(np.int64))
    assert (docs == 0).sum() > 5 and large.doc_chunk_off[0] == 0 and large.doc_chunk_off[-1] == len(lens)
    assert large.doc_off[-1] == len(large.data)
    # the singles are the NUL-led chunks with a number, and some NUL-led chunks are none
    nul_led = [c for c in large.chunks() if c[:1] == b"\x00"]
    assert len(nul_led) > L["singles"] == 300 and Mc["singles"] == 3
    assert all(i < 65536 for _, _, i in HC.nul_singles("large"))
    # one chunk above the deduper's limit, equal and distinct stretches
    assert lens.max() > 256 and HC.dedup_counts("large", 256)[1] < HC.dedup_counts("large", 0)[1] == L["chunks"]
    # ones: more chunk ends than the idle token array holds (8 bytes an end, 4 bytes a text byte)
    one = HC.pool()["ones"]
    assert (np.diff(one.chunk_off.astype(np.int64)) == 1).all() and len(one.data) >= len(large.data)
    # small: every length, one document, one chunk or a last end inside a 32-bit mask word
    assert [len(HC.pool()[n].data) for n in HC.SMALL] == list(HC.SMALL_LENGTHS)
    for name in HC.SMALL:
        inp = HC.pool()[name]
        assert inp.n_docs == 1 and (len(inp.chunk_off) == 2 or len(inp.data) % 32)
        assert not HC.nul_singles(name)
    # the table: what mbpe_merges_check accepts, under 65,536 ids, with pairs over the markers' ids
    m = HC.merges()
    assert R.well_formed(m) and HC.n_table_ids() < 65536
    ids = {i for _, _, i in HC.nul_singles("large")}
    assert ids == {0, 7, 12, 49, 300} and all(any(i in pair for pair in m.tolist()) for i in ids)


# ---- the references ---------------------------------------------------------------------------------------------------------

def test_greedy_reference_equals_the_oracle_and_rank_references_agree():
    m = HC.merges()
    for name, inp in HC.pool().items():
        data = np.frombuffer(inp.data, dtype=np.uint8)
        greedy, boff = B.encode_chunks(inp.data, inp.chunk_off, m, rank=False)
        assert np.array_equal(greedy, O.encode_chunks(data, inp.chunk_off, m)), name
        tok, end, pos = HC.stream(name, "greedy", None, "nul")
        assert np.array_equal(tok, greedy) and np.array_equal(D.byte_offsets(pos, len(data)), boff), name
        # rank order three ways: chunk by chunk with positions, the whole text in numpy, dropout at p = 0
        rank, rank_boff = B.encode_chunks(inp.data, inp.chunk_off, m, rank=True)
        text_tok, text_end, _ = R.reference(R.RankCase(data, inp.chunk_off, m, name))
        drop_tok, drop_end, drop_pos, _ = D.reference(inp.data, inp.chunk_off, m, 99, 0)
        tok, end, pos = HC.stream(name, "rank", None, "nul")
        for other in (rank, text_tok, drop_tok):
            assert np.array_equal(tok, other), name
        assert np.array_equal(end, text_end) and np.array_equal(end, drop_end), name
        assert np.array_equal(pos, drop_pos) and np.array_equal(D.byte_offsets(pos, len(data)), rank_boff), name
        assert np.array_equal(HC.stream(name, "rank", (0.0, 5), "nul")[0], tok), name
    # singles given as rows are the NUL rule's tokens where the rows are the NUL rule's chunks
    for name in ("large", "medium"):
        for order in ("greedy", "rank"):
            a, b = HC.stream(name, order, None, "nul"), HC.stream(name, order, None, HC.nul_singles(name))
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (name, order)
        a = HC.stream(name, "rank", (0.3, 5), "nul")
        b = HC.stream(name, "rank", (0.3, 5), HC.nul_singles(name))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a[0]) > len(HC.stream(name, "rank", None, "nul")[0])


def test_expected_depends_on_the_step_alone():
    sched = HC.hand_made("stages_toggle")
    first = [HC._expected(s) for s in sched.steps[:4]]
    for s in reversed(sched.steps):
        HC._expected(s)
    again = [HC._expected(s) for s in sched.steps[:4]]
    for a, b in zip(first, again):
        assert sorted(a) == sorted(b)
        for k in a:
            assert HC._same(k, b[k], a[k]) is None, k


# ---- the checker catches history dependence -----------------------------------------------------------------------------------

def _ends(inp):
    lens = np.diff(inp.chunk_off.astype(np.int64))
    return set((inp.chunk_off[1:][lens > 0].astype(np.int64) - 1).tolist())


def predict(defect, sched):
    """The first step at which the defect must show, from the schedule alone; None: it never does."""
    pool, steps = HC.pool(), sched.steps
    for i, st in enumerate(steps):
        inp, earlier = pool[st.inp], steps[:i]
        ok = HC.refusal(st) is None
        n = len(inp.data)
        if defect == "stale_mask" and ok:
            for p in range(n, -(-n // 32) * 32):                    # the rest of the last mask word
                wrote = [e for e in earlier if len(pool[e.inp].data) > p]
                if wrote and p in _ends(pool[wrote[-1].inp]):
                    return i
        if defect == "stale_singles" and ok:
            mine = set(HC._singles_key(st) if st.endmask else HC.nul_singles(st.inp))
            for e in earlier:
                for r in (HC._singles_key(e) if e.endmask else HC.nul_singles(e.inp)):
                    if r[0] + r[1] <= n and r not in mine:
                        return i
        if defect == "stale_docs" and ok and st.route in HC.BATCH:
            if any(pool[e.inp].n_docs > inp.n_docs for e in earlier if e.route in HC.BATCH):
                return i
        if defect == "stale_stage" and st.route in HC.BATCH:
            kept = {k: st.set[k] if st.set[k] is not None else
                    next((e.set[k] for e in reversed(earlier) if e.set[k] is not None), None) for k in ("fim", "mlm")}
            if kept != {k: st.set[k] for k in kept}:
                import dataclasses
                other = HC.expected(dataclasses.replace(st, set=dict(st.set, **kept)))
                mine = HC.expected(st)
                if sorted(other) != sorted(mine) or any(HC._same(k, other[k], mine[k]) for k in mine if k != "delta"):
                    return i
        if defect == "wide_store" and ok and st.bits == 16 and st.cap != "query":
            want = HC.expected(st)
            a = want.get("tokens", want.get("ids"))
            if a is not None and (a.size >= 2 or (a.size == 1 and st.out == "dev")):
                return i
    return None


def first_failure(defect, sched):
    enc, judge = HC.StandIn(defect), HC.Judge(sched)
    for i, step in enumerate(sched.steps):
        try:
            judge.check(i, enc.run(step))
        except HC.Mismatch as e:
            assert "schedule %s, step %d of" % (sched.name, i) in str(e) and step.describe() in str(e)
            assert str(e).count("\n    step ") == min(i, 3)          # the message names the three steps before it
            return i
    return None


@pytest.mark.parametrize("name", HAND)
def test_a_correct_stand_in_passes(name):
    assert first_failure(None, HC.hand_made(name)) is None


# the schedule that was written around each kind of state, and the step at which that state must show
MADE_FOR = {"stale_mask": "mask_tail", "stale_singles": "singles_shrink", "stale_docs": "docs_shrink",
            "stale_stage": "stages_toggle", "wide_store": "widths_and_sides"}


@pytest.mark.parametrize("defect", HC.DEFECTS)
def test_the_checker_catches_a_stale_state_defect(defect):
    caught = {}
    for name in HAND:
        sched = HC.hand_made(name)
        want = predict(defect, sched)
        assert first_failure(defect, sched) == want, (defect, name)
        caught[name] = want
    at = caught[MADE_FOR[defect]]
    sched = HC.hand_made(MADE_FOR[defect])
    assert at is not None
    step = sched.steps[at]
    if defect == "stale_mask":          # the first small text whose length is no multiple of 32, behind the text of all ends
        assert step.inp == "s1" and all(s.inp in ("ones", "s0") for s in sched.steps[:at])
    elif defect == "stale_singles":     # the medium text behind the large one: 3 singles where there were 300
        assert step.inp == "medium" and all(s.inp == "large" for s in sched.steps[:at])
    elif defect == "stale_docs":        # the first call with one document
        assert step.inp == "s33" and all(s.inp == "large" for s in sched.steps[:at])
    elif defect == "stale_stage":       # the first call with FIM taken back
        assert step.set["fim"] is None and all(s.set["fim"] is not None for s in sched.steps[:at])
    else:                                # the first 16-bit output
        assert step.bits == 16 and all(s.bits == 32 for s in sched.steps[:at])


@pytest.mark.parametrize("seed", HC.SEEDS[:2])
def test_the_checker_catches_defects_in_constructed_schedules_too(seed):
    sched = HC.constructed(seed)
    assert first_failure(None, sched) is None
    for defect in HC.DEFECTS:
        want = predict(defect, sched)
        assert want is not None and first_failure(defect, sched) == want, defect


def test_the_guards_are_checked():
    step = HC.hand_made("widths_and_sides").steps[0]
    want = HC.expected(step)
    got = {k: v for k, v in want.items()}
    got["guards"] = {"tokens": np.full(HC.GUARD, HC.SENTINEL[4], dtype=np.uint32)}
    HC.check(step, got, want)
    got["guards"]["tokens"][HC.GUARD - 1] = 0
    with pytest.raises(HC.Mismatch, match="guard of tokens: 1 elements overwritten, the first at \\+63"):
        HC.check(step, got, want)
    del got["guards"]
    got["tokens"] = want["tokens"].astype(np.uint64)
    with pytest.raises(HC.Mismatch, match="tokens: got uint64"):
        HC.check(step, got, want)
    got["tokens"] = want["tokens"][:-1]
    with pytest.raises(HC.Mismatch, match="tokens: got uint32"):
        HC.check(step, got, want)
    got["tokens"] = want["tokens"]
    got["extra"] = 1
    with pytest.raises(HC.Mismatch, match="extra: not expected"):
        HC.check(step, got, want)


# ---- the Tokenizer's list -------------------------------------------------------------------------------------------------

def test_tokenizer_calls_turn_every_option_on_off_and_on():
    calls = HC.tokenizer_calls()
    assert len(calls) == 24
    assert {c[0] for c in calls} == {"encode", "encode_batch", "encode_batch_padded", "encode_batch_aux",
                                     "encode_batch_windows", "encode_batch_fit", "token_counts"}
    for option in ("order", "dropout", "dedup", "fim", "mlm", "device_split"):
        present = [option in kw for _, _, kw in calls]
        runs = [v for k, v in enumerate(present) if k == 0 or v != present[k - 1]]
        assert any(runs[k:k + 3] == [True, False, True] for k in range(len(runs))), option
        # a call without the option right behind a call with it: the place where a setting that is not re-set shows
        assert any(a and not b for a, b in zip(present[:-1], present[1:])), option
    for method, name, kw in calls:
        assert not (kw.get("dropout") and (kw.get("order") != "rank" or kw.get("dedup")))      # no refusal in this list
        assert not (kw.get("fim") and kw.get("mlm"))
        HC.tokenizer_expected(method, name, kw)


def test_the_ascii_restatement_of_the_gpt4_split_equals_the_host_splitter():
    """history_cases.gpt4_chunks judges the Tokenizer's calls; the library's host splitter (PCRE2, the pattern as the
    model file has it) is no judge there, but it must agree on ASCII text."""
    import mbpe
    from conftest import read_data, read_golden
    pattern = B.parse_model(read_golden(HC.MODEL + ".model"))[0]
    for name in ("taylorswift.txt", "shakespeare.txt"):
        text = bytes(c for c in read_data(name)[:200000] if 0 < c < 128)
        assert HC.gpt4_chunks(text) == mbpe.presplit_ranges(pattern, text)[1].tolist(), name
    for texts in HC.tokenizer_texts().values():
        for t in texts:
            for a, b, sid in (B.split_special(t, HC.tokenizer_specials()) if t else []):
                if sid is None:
                    assert HC.gpt4_chunks(t[a:b]) == mbpe.presplit_ranges(pattern, t[a:b])[1].tolist()
