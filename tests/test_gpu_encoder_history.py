"""One long-lived mbpe.Encoder through schedules of calls of different kinds, sizes and settings (tests/history_cases.py),
every result checked against references in Python that depend on the call alone: the result of an encoder call is a
function of its arguments and the settings in force, never of the calls made before it.  The encoder keeps about fifty
device buffers, grown on demand, some borrowed across roles, and a dozen settings and host-side lists; fresh device
memory is usually zero, so a kernel that reads behind its input, a mask tail, an offset array that is not rewritten or
a list that is not cleared shows only after a LARGER call has gone before.  That is the order the schedules are made of.

Device texts are followed by 0xFF bytes, the caller's end mask is built to the header's layout with 0xFF behind it in
the same allocation, every device output is prefilled with a sentinel and GUARD elements longer than it needs to be."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import history_cases as HC
import mbpe

pytestmark = pytest.mark.gpu

_INT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


@pytest.fixture(scope="module")
def device():
    torch.cuda.set_device(0)
    return Device(torch.device("cuda", 0))


class Device:
    """The pool in device memory: every text at a 16-byte boundary and one byte behind one, every end mask."""

    def __init__(self, dev):
        self.dev = dev
        self.text, self.text1, self.mask = {}, {}, {}
        for name, inp in HC.pool().items():
            data = np.frombuffer(inp.data, dtype=np.uint8)
            tail = np.full(64, 0xFF, dtype=np.uint8)
            self.text[name] = self.upload(np.concatenate([data, tail]))
            self.text1[name] = self.upload(np.concatenate([tail[:1], data, tail]))
            mask = HC.end_mask(inp)
            assert len(mask) == 2 * ((len(data) + 15) // 16) + 16
            self.mask[name] = self.upload(np.concatenate([mask, tail]))
        torch.cuda.synchronize()

    def upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).view(_INT[a.dtype.itemsize]).copy()).to(self.dev)

    def text_ptr(self, step):
        t = self.text1[step.inp] if step.text == "dev1" else self.text[step.inp]
        assert t.data_ptr() % 16 == 0
        return t.data_ptr() + (1 if step.text == "dev1" else 0)

    def output(self, n, dtype):
        """n + GUARD elements of the sentinel -> the tensor"""
        dtype = np.dtype(dtype)
        a = np.full(n + HC.GUARD, HC.SENTINEL[dtype.itemsize], dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[dtype.itemsize])
        return self.upload(a)


def read(t, dtype):
    return t.cpu().numpy().view(dtype)


class Runner:
    """Makes the call of a step on one encoder -> what check() takes.  Only the settings that differ from those in force
    are applied: a setting left over from an earlier step is part of what is tested."""

    def __init__(self, enc, device):
        self.enc, self.device, self.cur = enc, device, dict(HC.DEFAULTS)
        self.n_calls = 0

    def apply(self, step):
        enc, cur, new = self.enc, self.cur, step.set
        if step.route == "count" and step.reset:
            enc.reset_counts()
        if new["order"] != cur["order"]:
            enc.set_option("rank_order", int(new["order"] == "rank"))
        if new["dropout"] != cur["dropout"]:
            enc.set_dropout(*(new["dropout"] or (0.0, 0)))
        if new["dedup"] != cur["dedup"]:
            enc.set_option("dedup", int(new["dedup"]))
        if new["dedup_max"] != cur["dedup_max"]:
            enc.set_option("dedup_max_chunk_bytes", new["dedup_max"])
        if new["piece_bytes"] != cur["piece_bytes"]:
            enc.set_option("piece_bytes", new["piece_bytes"])
        if new["fim"] != cur["fim"]:
            enc.set_fim(None if new["fim"] is None else fim_spec(new["fim"]))
        if new["mlm"] != cur["mlm"]:
            enc.set_mlm(None if new["mlm"] is None else mlm_spec(new["mlm"]))
        if new["count_ids"] != cur["count_ids"]:
            enc.set_option("count_ids", new["count_ids"])
        self.cur = dict(new)

    def run(self, step):
        self.apply(step)
        self.guards = {}
        torch.cuda.synchronize()
        got = {}
        call = self.count if step.route == "count" else self.batch if step.route in HC.BATCH else self.flat
        self.enc.n_out = self.enc.n_rows = self.enc.n_tokens = None       # (what the binding notes of a call)
        try:
            call(step, got)
            got["error"] = HC.OK
        except mbpe.MbpeError as e:
            # a refused call: its code, the counts it still reports, and every device buffer as it was
            got = {"error": e.code}
            if step.route in HC.BATCH:
                got["n_rows"], got["n_tokens"] = getattr(self.enc, "n_rows", None), self.enc.n_tokens
            else:
                got["n_out"] = getattr(self.enc, "n_out", None)
            for name, (t, dtype, n) in self.guards.items():
                self.guards[name] = (t, dtype, 0)
        self.n_calls += 1
        if step.route == "count":
            got["counts"] = self.enc.counts()
        if got["error"] == HC.OK:
            try:
                st = self.enc.dedup_stats()
                got["dedup_stats"] = (st["n_chunks"], st["n_unique"], st["n_unique_bytes"])
            except mbpe.MbpeError as e:
                got["dedup_stats"] = e.code
        if self.guards:
            torch.cuda.synchronize()
            got["guards"] = {}
            for name, (t, dtype, n) in self.guards.items():
                a = read(t, dtype)
                if got["error"] == HC.OK:
                    got[name] = a[:n].copy()
                got["guards"][name] = a[n:].copy()
        return got

    # -- what the calls take

    def out(self, name, n, dtype):
        """A device output of n elements: its pointer; it is read back, split at n into result and guard, after the call"""
        t = self.device.output(n, dtype)
        torch.cuda.synchronize()
        self.guards[name] = (t, np.dtype(dtype), n)
        return t.data_ptr()

    def sizes(self, step):
        """What the call needs, to give it exactly that: from the reference of the same call with room enough (a wrong
        reference makes the call fail, it cannot make it pass)."""
        want = HC.expected(dataclasses.replace(step, cap="n"))
        n_bytes = len(HC.pool()[step.inp].data)
        batch = step.route in HC.BATCH
        n = want.get("n_rows" if batch else "n_out")
        return ((1 if batch else max(n_bytes, 1)) if n is None else n), -1 if step.cap == "short" else 0

    def singles(self, step):
        rows = HC._singles_key(step)
        return [tuple(r) for r in rows] or None

    # -- the flat calls: plain, byteoff, endmask

    def flat(self, step, got):
        enc, inp = self.enc, HC.pool()[step.inp]
        n_bytes = len(inp.data)
        data = np.frombuffer(inp.data, dtype=np.uint8)
        dtype = np.uint16 if step.bits == 16 else np.uint32
        n, less = self.sizes(step)
        cap = max(n + less, 0)
        on_dev = step.text != "host"
        tp = self.device.text_ptr(step) if on_dev else (data.ctypes.data if n_bytes else 0)
        if step.endmask:
            head = (tp, n_bytes, self.device.mask[step.inp].data_ptr())
            kw = dict(singles=self.singles(step), doc_off=inp.doc_off if step.docs else None, dtype=dtype)
            if step.cap == "query":
                res = enc.encode_endmask(*head, query=True, **kw)
            elif step.out == "dev":
                res = enc.encode_endmask(*head, out_ptr=self.out("tokens", n, dtype), cap=cap,
                                         byte_off_ptr=self.out("byte_off", n + 1, np.uint64) if step.byteoff else None, **kw)
            else:
                res = enc.encode_endmask(*head, cap=cap, byte_off=step.byteoff, **kw)
                got["tokens"] = res[0]
                if step.byteoff:
                    got["byte_off"] = res[2]
            got["n_out"] = res[0] if isinstance(res[0], int) else len(res[0])
            if step.docs:
                got["doc_tok_off"] = res[1]
            else:
                assert res[1] is None
            return
        off = inp.chunk_off
        if step.cap == "query" or step.out == "dev":
            query = step.cap == "query"
            res = enc.encode_device(tp, n_bytes, off, 0 if query else self.out("tokens", n, dtype), 0 if query else cap,
                                    token_bits=step.bits, offsets=step.offsets, text_on_device=on_dev,
                                    byte_off_ptr=self.out("byte_off", n + 1, np.uint64) if step.byteoff and not query else None)
            got["n_out"], tok_off = res if step.offsets else (res, None)
        else:
            res = enc.encode(None if on_dev else data, off, offsets=step.offsets, dtype=dtype, byte_off=step.byteoff,
                             text_ptr=tp if on_dev else None, n_bytes=n_bytes if on_dev else None, cap=cap)
            res = res if isinstance(res, tuple) else (res,)
            got["tokens"], got["n_out"] = res[0], len(res[0])
            tok_off = res[1] if step.offsets else None
            if step.byteoff:
                got["byte_off"] = res[-1]
        if step.offsets:
            got["chunk_tok_off"] = tok_off

    # -- the batch calls: pack, aux, windows, fit

    def batch(self, step, got):
        enc, inp, p = self.enc, HC.pool()[step.inp], step.pack
        n_bytes, S, bits = len(inp.data), step.pack["seq_len"], step.bits
        ids_t, lab_t = (np.uint16, np.uint16) if bits == 16 else (np.uint32, np.int32)
        n_rows, less = self.sizes(step)
        query, on_dev = step.cap == "query", step.out == "dev" or step.cap == "query"
        kw = dict(seq_len=S, out_bits=bits, pad_id=p["pad"], bos_id=p["bos"], eos_id=p["eos"])
        if step.route in ("pack", "aux"):
            kw.update(layout=p["layout"], pad_left=p["pad_left"], trunc_left=p["trunc_left"])
        if step.route != "pack":
            kw.update(ignore_label=HC.IGNORE[bits])
        if step.route == "windows":
            kw.update(stride=p["stride"], score_once=p["score_once"])
        if on_dev:
            cells = n_rows * S
            kw.update(out_ptr=0 if query else self.out("ids", cells, ids_t), cap_rows=0 if query else max(n_rows + less, 0),
                      len_ptr=None if query else self.out("lengths", n_rows, np.uint32))
            if step.route != "pack" and not query:
                kw.update(labels_ptr=self.out("labels", cells, lab_t), pos_ptr=self.out("positions", cells, np.uint32),
                          seg_ptr=self.out("segments", cells, np.uint32))
            if step.route == "windows" and not query:
                kw.update(row_doc_ptr=self.out("row_doc", n_rows, np.uint32), row_tok0_ptr=self.out("row_tok0", n_rows, np.uint64))
            if step.route == "fit" and not query:
                kw.update(doc_row_ptr=self.out("doc_row", inp.n_docs, np.uint64), doc_col_ptr=self.out("doc_col", inp.n_docs, np.uint32))
        else:
            if step.route != "pack":
                kw.update(labels=True, positions=True, segments=True)
            if step.route == "windows":
                kw.update(row_doc=True, row_tok0=True)
            if step.route == "fit":
                kw.update(doc_row=True, doc_col=True)
        if step.endmask:
            head = (self.device.text_ptr(step), n_bytes, self.device.mask[step.inp].data_ptr(), self.singles(step), inp.doc_off)
            fn = {"pack": enc.encode_batch_endmask, "aux": enc.encode_batch_endmask, "windows": enc.encode_batch_endmask_windows,
                  "fit": enc.encode_batch_endmask_fit}[step.route]
        else:
            if step.text == "host":
                head = (np.frombuffer(inp.data, dtype=np.uint8), inp.chunk_off, inp.doc_chunk_off)
            else:
                head = (None, inp.chunk_off, inp.doc_chunk_off)
                kw.update(text_ptr=self.device.text_ptr(step), n_bytes=n_bytes)
            fn = {"pack": enc.encode_batch, "aux": enc.encode_batch_aux, "windows": enc.encode_batch_windows,
                  "fit": enc.encode_batch_fit}[step.route]
        res = fn(*head, **kw)
        if on_dev:
            got["n_rows"] = res
        elif step.route == "pack":
            got["ids"], got["lengths"] = res
            got["n_rows"] = len(res[0])
        else:
            for k in ("ids", "lengths", "labels", "positions", "segments", "row_doc", "row_tok0", "doc_row", "doc_col"):
                if k in res:
                    got[k] = res[k]
            got["n_rows"] = len(res["ids"])
        got["n_tokens"] = enc.n_tokens
        if step.route != "pack":
            got["doc_tok_off"] = enc.doc_tok_off
            # cu_seqlens is host arithmetic on the offsets the call handed back
            if step.route == "fit":
                cu, longest = mbpe.pack_fit_cu_seqlens(enc.doc_tok_off, S, p["bos"], p["eos"])
                got["cu_seqlens"], got["max_seqlen"] = cu, longest
            elif step.route == "aux" and p["layout"] == "packed":
                cu, longest = mbpe.pack_cu_seqlens(enc.doc_tok_off, S, p["bos"], p["eos"])
                got["cu_seqlens"], got["max_seqlen"] = cu, longest
        got["fim_info"] = enc.fim_info()

    # -- count

    def count(self, step, got):
        enc, inp = self.enc, HC.pool()[step.inp]
        n_bytes = len(inp.data)
        if step.endmask:
            got["n_out"] = enc.count_endmask(self.device.text_ptr(step), n_bytes, self.device.mask[step.inp].data_ptr(),
                                             self.singles(step), repeat=step.repeat)
        elif step.text == "host":
            got["n_out"] = enc.count(np.frombuffer(inp.data, dtype=np.uint8), inp.chunk_off, repeat=step.repeat)
        else:
            got["n_out"] = enc.count_device(self.device.text_ptr(step), n_bytes, inp.chunk_off, repeat=step.repeat)


def finish(step, got):
    """the matrices of a device call come back flat: give them the shape the call reported"""
    if step.route in HC.BATCH and got["error"] == HC.OK and "n_rows" in got:
        S = step.pack["seq_len"]
        for name in ("ids", "labels", "positions", "segments"):
            if name in got and got[name].ndim == 1:
                got[name] = got[name].reshape(-1, S)
    return got


def run_schedule(sched, device, enc=None):
    own = enc is None
    enc = mbpe.Encoder(HC.merges()) if own else enc
    try:
        runner, judge = Runner(enc, device), HC.Judge(sched)
        results = []
        for i, step in enumerate(sched.steps):
            got = finish(step, runner.run(step))
            judge.check(i, got)
            results.append(got)
        assert runner.n_calls == len(sched.steps) == len(results)
        return results
    finally:
        if own:
            enc.close()


# ---- the tests ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [f.__name__ for f in HC.HAND_MADE])
def test_hand_made(device, name):
    run_schedule(HC.hand_made(name), device)


@pytest.mark.parametrize("seed", HC.SEEDS)
def test_constructed(device, seed):
    run_schedule(HC.constructed(seed), device)


def _equal(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def test_fresh_encoder_agrees(device):
    """Every step of the first constructed schedule again on an encoder of its own: where the long-lived encoder fails
    the reference and the fresh one does not, the fault is history, not the feature.  (The count table accumulates by
    contract: the two are compared on everything else.)"""
    sched = HC.constructed(HC.SEEDS[0])
    with mbpe.Encoder(HC.merges()) as enc:
        old = Runner(enc, device)
        for i, step in enumerate(sched.steps):
            got = finish(step, old.run(step))
            with mbpe.Encoder(HC.merges()) as fresh:
                new = finish(step, Runner(fresh, device).run(dataclasses.replace(step, reset=False)))
            got.pop("counts", None)
            new.pop("counts", None)
            assert _equal(got, new), "step %d: %s\n  the long-lived encoder and a fresh one differ in %s" % (
                i, step.describe(), [k for k in got if k not in new or not _equal(got[k], new[k])])


def test_allocations_settle(device):
    """docs_shrink twice on one encoder: the second run meets no size and no kind of call that the first did not, so it
    allocates nothing -- "a repeat call of no larger size allocates nothing", across kinds."""
    sched = HC.hand_made("docs_shrink")
    with mbpe.Encoder(HC.merges()) as enc:
        run_schedule(sched, device, enc)
        first = enc.alloc_count()
        run_schedule(sched, device, enc)
        assert enc.alloc_count() == first


# ---- one Tokenizer --------------------------------------------------------------------------------------------------------

def test_tokenizer_history():
    """One mbpe.Tokenizer, 24 calls, the options given per call: every result is the reference's, so an option a call does
    not name is off for it whatever the call before it named (host/tokenizer.cpp keeps one encoder and re-sets it)."""
    import byteoff_cases as B
    from conftest import read_data, read_golden
    pattern, _ = B.parse_model(read_golden(HC.MODEL + ".model"))
    tok = mbpe.Tokenizer(pattern)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    tok.set_merges(HC.merges())
    calls = HC.tokenizer_calls()
    assert len(calls) == 24
    try:
        for i, (method, name, kw) in enumerate(calls):
            what = "call %d: %s(%s, %s)" % (i, method, name, sorted(kw))
            texts = HC.tokenizer_texts()[name]
            want = HC.tokenizer_expected(method, name, kw)
            kw = dict(kw)
            for k, make in (("fim", fim_spec), ("mlm", mlm_spec)):
                if k in kw:
                    kw[k] = make(kw[k])
            if method == "encode":
                got = tok.encode(b"".join(texts), device=0, **kw)
                assert got.dtype == np.uint32 and np.array_equal(got, want), what
            elif method == "encode_batch":
                got = tok.encode_batch(texts, **kw)
                assert [g.tolist() for g in got] == [w.tolist() for w in want], what
            elif method == "token_counts":
                got = tok.token_counts(texts, **kw)
                assert got.dtype == np.uint64 and np.array_equal(got, want), what
            else:
                got = getattr(tok, method)(texts, **HC.TOK_PACK, **kw)
                if method == "encode_batch_padded":
                    got = {"ids": got[0], "lengths": got[1]}
                else:
                    got["doc_tok_off"] = tok.doc_tok_off
                try:
                    HC.check(None, dict(got, error=HC.OK), dict(want, error=HC.OK))
                except HC.Mismatch as e:
                    raise AssertionError("%s: %s" % (what, e)) from None
    finally:
        tok.close()


def fim_spec(f):
    return mbpe.FimSpec(f["rate"], f["spm"], f["seed"], f["doc_base"], f["pre"], f["suf"], f["mid"], f["min_tokens"],
                        f["max_tokens"])


def mlm_spec(m):
    return mbpe.MlmSpec(m["select"], m["mask"], m["random"], m["seed"], m["doc_base"], m["mask_id"], m["vocab_n"],
                        m["whole_word"], len(m["protect"]), (ctypes.c_uint32 * 8)(*m["protect"]))
