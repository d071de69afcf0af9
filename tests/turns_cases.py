"""The rule of multi-turn conversation batches (include/mbpe.h, mbpe_turns_spec) in plain Python lists: the full stream
of a conversation is built id by id with a trained bit, then truncated.  It shares no code with the library;
tests/test_turns_cpu.py and tests/test_gpu_turns.py compare the library with it."""
NONE = 0xFFFFFFFF
TRAIN, NO_END = 1, 2
TRUNCATIONS = ("right", "left", "drop_oldest")
LABELS = ("all", "trained")


def full_stream(turns, flags, turn_end_id, end_id):
    """The turns (token lists) of one conversation -> (ids with their trained bits, one list per turn; the end ids)."""
    per_turn = []
    for toks, f in zip(turns, flags):
        ids = [(t & 0x7FFFFFFF, bool(f & TRAIN)) for t in toks]
        if turn_end_id is not None and not f & NO_END:
            ids.append((turn_end_id, bool(f & TRAIN)))
        per_turn.append(ids)
    end = [] if end_id is None else [(end_id, bool(turns) and bool(flags[-1] & TRAIN))]
    return per_turn, end


def join(turns, flags, max_tokens=0, truncation="right", head_turns=0, turn_end_id=None, end_id=None, labels="trained"):
    """One conversation -> (kept ids, targets, (dropped, cut)); the keywords are those of mbpe.turns_spec."""
    per_turn, end = full_stream(turns, flags, turn_end_id, end_id)
    flat = lambda ts: [x for t in ts for x in t]
    stream, dropped, cut, K, m = flat(per_turn) + end, 0, 0, max_tokens, len(turns)
    if K and truncation == "right":
        stream, cut = stream[:K], len(stream) - min(len(stream), K)
    elif K and truncation == "left":
        cut = len(stream) - min(len(stream), K)
        stream = stream[cut:]
    elif K:
        h = min(head_turns, m)
        F = lambda j: len(flat(per_turn[:h])) + len(flat(per_turn[j:])) + len(end)
        j = next((j for j in range(h, m + 1) if F(j) <= K), m)
        while j < m and flags[j] & TRAIN:
            j += 1
        stream = flat(per_turn[:h]) + flat(per_turn[j:]) + end
        dropped, cut = j - h, len(stream) - min(len(stream), K)
        stream = stream[:K]
    ids = [i for i, _ in stream]
    tgt = [ids[k + 1] if k + 1 < len(ids) and (labels == "all" or stream[k + 1][1]) else NONE for k in range(len(ids))]
    return ids, tgt, (dropped, cut)


def join_all(docs, turn_off, flags, **kw):
    """The turns docs (token lists) by conversation -> (flat ids, flat targets, offsets, info)."""
    flat, tgt, off, info = [], [], [0], []
    for c in range(len(turn_off) - 1):
        a, b = int(turn_off[c]), int(turn_off[c + 1])
        ids, t, dc = join(docs[a:b], [int(f) for f in flags[a:b]], **kw)
        flat += ids
        tgt += t
        off.append(len(flat))
        info.append(list(dc))
    return flat, tgt, off, info
