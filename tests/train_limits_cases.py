"""Training under the stopping rules "min_frequency" and "max_token_length", restated in Python: the reference of
tests/test_train_limits_cpu.py and of the GPU tests (test_gpu_train_limits.py, test_gpu_train_limits_tokenizer.py).

The rules.  len[i] = 1 for a byte, len[256 + k] = len[a_k] + len[b_k]; the merges a continued training starts from
count too.  With max_token_length L > 0 a pair (a, b) is ELIGIBLE iff len[a] + len[b] <= L; ineligible pairs stay in
the stream and the table and are counted as ever, and are never chosen.  One step: M is the largest count among the
eligible pairs of the table (lexical: the never-erased table, zero counts included; first: what a recount gives).
The training ends when no pair is eligible, when M < min_frequency, or (first) when M == 0; otherwise lexical takes
the eligible pair of count M with the smallest (first, second), first the one whose first occurrence is earliest."""
import dedup_cases as C

SPAN = 1024      # tokens one wave of the device's position search walks


def limited_bpe(chunks, weights, vocab_size, first_mode, L=0, f=0, start=None, trace=True):
    """dedup_cases.weighted_bpe under the rules above -> (merges, counts, trace).
    start: (sequences, n, prior merges) -- the prior merges give the lengths of ids 256 .. 255 + n; (sequences, n) will
    do while L == 0.
    trace: one dict per step made, saying whether an ineligible pair had
      "larger"        a larger count than the winner,
      "smaller_key"   the same count and a smaller (first, second),
      "earlier_span"  the same count and an earlier first position, in another SPAN-token span of the stream;
    trace=False skips that bookkeeping (and returns an empty list), for long inputs.
    The table is kept incrementally in both modes: its non-zero entries are what a recount gives (test_train_limits_cpu
    checks that against weighted_bpe, which recounts)."""
    if start is None:
        seqs, k0, prior = [list(c) for c in chunks], 0, []
    else:
        seqs, k0 = [list(s) for s in start[0]], int(start[1])
        prior = [tuple(int(x) for x in p) for p in start[2]] if len(start) > 2 else None
    if prior is None:
        if L and k0:
            raise ValueError("a length limit on a continued training needs the prior merges")
        length = [1] * (256 + k0)
    else:
        assert len(prior) == k0
        length = [1] * 256
        for a, b in prior:
            length.append(length[a] + length[b])

    def eligible(key):
        return L == 0 or length[key[0]] + length[key[1]] <= L

    def first_positions(only=None):
        """first stream position of every pair (of the pairs in `only`: stops once each is found)"""
        pos, p = {}, 0
        for s in seqs:
            for i in range(len(s) - 1):
                key = (s[i], s[i + 1])
                if key not in pos and (only is None or key in only):
                    pos[key] = p + i
                    if only is not None and len(pos) == len(only):
                        return pos
            p += len(s)
        return pos

    tab = {}
    for s, w in zip(seqs, weights):
        for i in range(len(s) - 1):
            key = (s[i], s[i + 1])
            tab[key] = tab.get(key, 0) + int(w)
    merges, counts, steps = [], [], []
    for k in range(k0, vocab_size - 256):
        live = {key: c for key, c in tab.items() if c > 0} if first_mode else tab
        elig = {key: c for key, c in live.items() if eligible(key)}
        if not elig:
            break
        top = max(elig.values())
        if top < f or (first_mode and top == 0):
            break
        tied = [key for key, c in elig.items() if c == top]
        pos = first_positions() if trace else None
        if first_mode and len(tied) > 1:
            if pos is None:
                pos = first_positions(set(tied))
            win = min((pos[key], key) for key in tied)[1]
        else:
            win = min(tied)
        if trace:
            out = [(key, c) for key, c in live.items() if not eligible(key)]
            steps.append({
                "larger": any(c > top for _, c in out),
                "smaller_key": any(c == top and key < win for key, c in out),
                "earlier_span": win in pos and any(c == top and key in pos and pos[key] // SPAN < pos[win] // SPAN
                                                   for key, c in out),
            })
        a, b = win
        merges.append(win)
        counts.append(top)
        X = 256 + k
        length.extend([0] * (X + 1 - len(length)))
        length[X] = length[a] + length[b]
        for n, (s, w) in enumerate(zip(seqs, weights)):
            if a not in s:
                continue
            w = int(w)
            new, i = [], 0
            while i < len(s):
                if i + 1 < len(s) and s[i] == a and s[i + 1] == b:
                    tab[(a, b)] = tab.get((a, b), 0) - w
                    if new:
                        x = new[-1]
                        tab[(x, a)] = tab.get((x, a), 0) - w
                        tab[(x, X)] = tab.get((x, X), 0) + w
                    if i + 2 < len(s):
                        y = s[i + 2]
                        tab[(b, y)] = tab.get((b, y), 0) - w
                        tab[(X, y)] = tab.get((X, y), 0) + w
                    new.append(X)
                    i += 2
                else:
                    new.append(s[i])
                    i += 1
            seqs[n] = new
    return merges, counts, steps


def token_lengths(merges):
    """byte length of every token id 0 .. 255 + len(merges)"""
    length = [1] * 256
    for a, b in merges:
        length.append(length[int(a)] + length[int(b)])
    return length


def apply_merges(chunks, merges):
    """The chunks as token sequences after `merges`, each applied as the training's walk applies it."""
    seqs = [list(c) for c in chunks]
    for k, (a, b) in enumerate(merges):
        a, b, X = int(a), int(b), 256 + k
        for n, s in enumerate(seqs):
            if a not in s:
                continue
            new, i = [], 0
            while i < len(s):
                if i + 1 < len(s) and s[i] == a and s[i + 1] == b:
                    new.append(X)
                    i += 2
                else:
                    new.append(s[i])
                    i += 1
            seqs[n] = new
    return seqs


# ---- the constructed cases: (chunks, L, vocab_size, lexical merges, lexical counts, first merges) ---------------------
# A: after (a, b) the ineligible (256, c) ties with (d, e) at count 3 and stands at position 0; the winner lies beyond
#    the first span.  B: after (a, b) and (c, d) the ineligible (256, 256) ties with (257, e) and has the smaller key
#    and the earlier position.
CASE_A = ([b"abc"] * 3 + [b"z"] * 1100 + [b"de"] * 3, 2, 259,
          [(97, 98), (100, 101), (97, 98)], [3, 3, 0], [(97, 98), (100, 101)])
CASE_B = ([b"abab"] * 3 + [b"z"] * 1100 + [b"cde"] * 3, 3, 260,
          [(97, 98), (99, 100), (257, 101), (97, 98)], [6, 3, 3, 0], [(97, 98), (99, 100), (257, 101)])
# C: (a, b) occurs 5 times, (c, d) 4 times: min_frequency -> merges made
CASE_C = ([b"ab", b"cd"], [5, 4], 260, {5: 1, 4: 2, 6: 0})


def random_inputs(seed):
    """The random corpus of the parity tests: ~19,500 tokens over 1 + seed symbols -> (chunks, unique chunks, weights)."""
    chunks = C.random_chunks(100 + seed, 3000, 12, 1 + seed)
    uniq, weights, _ = C.dedup(chunks)
    return chunks, uniq, weights
