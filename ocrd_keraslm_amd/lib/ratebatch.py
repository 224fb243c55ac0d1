"""Scheduler of `Rater.rate_batch`: many independent texts as lockstep rows of stateful windows.

`Rater.rate` (rating.py:493-529) feeds ONE text as `1 x length` windows.  Texts that do not depend on each other
can share a window call instead: each of B rows carries one text at a time, the windows of a text are exactly those
of `windows.stateful_windows(text, context, length, c_i)` (`train=False`), in order and in one row, and a row whose
text is finished takes the next text at the next call with that row's state zeroed.  A row with nothing left carries
`idx 0 / tgt -1` (no target, no bits).

Texts are dealt longest first to the row that is free first (list scheduling), so the number of window calls is at
most ceil(sum N_i / B) + max N_i for texts of N_i windows (Graham's bound; it holds for any order of the list).

`Rater.rate_alternatives` runs the same plan and delivers, per character, also the model's k most probable characters and
the rank of the one written: `alternatives_of` states that selection in numpy, `Plan.text_alternatives` slices it per text.

numpy only: the plan is built and tested without an engine.
"""
from __future__ import annotations

import numpy as np

from . import ratebulk, windows


class Plan(object):
    """What `plan` returns.

    B, T        rows and window length of every call
    n_calls     number of window calls
    row, first, count   per text (input order): its row, its first call and its number of windows (0: none, row -1)
    sizes       per text: its number of characters
    """

    def __init__(self, B, T, n_calls, row, first, count, sizes, X, Y, Z, slots):
        self.B, self.T, self.n_calls = B, T, n_calls
        self.row, self.first, self.count, self.sizes = row, first, count, sizes
        self._X, self._Y, self._Z, self._slots = X, Y, Z, slots
        starts = [[] for _ in range(n_calls)]
        ends = [[] for _ in range(n_calls)]
        for i in np.nonzero(count > 0)[0]:
            starts[first[i]].append(int(i))
            ends[first[i] + count[i] - 1].append(int(i))
        self._starts, self._ends = starts, ends

    def call(self, s):
        """(idx [B,T], ctx [B,T,C], tgt [B,T]) int32 of call s"""
        w = self._slots[s]
        return self._X[w], self._Z[w], self._Y[w]

    def starting(self, s):
        """texts whose first window is in call s: their rows start from a zero state"""
        return self._starts[s]

    def ending(self, s):
        """texts whose last window is in call s"""
        return self._ends[s]

    def reset_rows(self, s):
        return [int(self.row[i]) for i in self._starts[s]]

    def text_probs(self, i, picked):
        """the probabilities of text i as `Rater.rate` lists them (1.0 for the first character) from the
        target probabilities of all calls, picked [n_calls][B][T]"""
        size = int(self.sizes[i])
        out = np.ones(min(size, 1) if self.count[i] == 0 else size, dtype=np.float32)
        if self.count[i]:
            a = int(self.first[i])
            out[1:] = picked[a:a + int(self.count[i]), int(self.row[i])].reshape(-1)[:size - 1]
        return out

    def text_alternatives(self, i, picked, rank, alt_id, alt_p):
        """text i's share of `Rater.rate_alternatives`, sliced as text_probs slices: (probs [n] f32, rank [n] i32,
        alt_ids [n,k] i32, alt_probs [n,k] f32) from the results of all calls -- picked, rank [n_calls][B][T] and alt_id,
        alt_p [n_calls][B][T][k].  The first character has no prediction: probability 1.0, rank -1, ids -1, probabilities 0."""
        k = alt_id.shape[-1]
        size = int(self.sizes[i])
        n = min(size, 1) if self.count[i] == 0 else size
        ranks = np.full(n, -1, dtype=np.int32)
        ids = np.full((n, k), -1, dtype=np.int32)
        probs = np.zeros((n, k), dtype=np.float32)
        if self.count[i]:
            a, c, r = int(self.first[i]), int(self.count[i]), int(self.row[i])
            ranks[1:] = rank[a:a + c, r].reshape(-1)[:size - 1]
            ids[1:] = alt_id[a:a + c, r].reshape(-1, k)[:size - 1]
            probs[1:] = alt_p[a:a + c, r].reshape(-1, k)[:size - 1]
        return self.text_probs(i, picked), ranks, ids, probs


ALTS_MAX = 8      # alternatives per position at most (KL_RATE_ALTS_MAX of the C ABI)


class RatedText(object):
    """One text of `Rater.rate_alternatives`, n characters:

    probs      [n] f32    probability of every character given its predecessors (1.0 for the first), as `rate_batch`
    rank       [n] i32    position of the character among all the model could have written there, 0 = its first choice
                          (-1 for the first character)
    alt_ids    [n,k] i32  the k most probable ids there, most probable first (-1: none -- first character, k > voc_size)
    alt_probs  [n,k] f32  their probabilities (0 where alt_ids is -1)
    """

    def __init__(self, probs, rank, alt_ids, alt_probs):
        self.probs, self.rank, self.alt_ids, self.alt_probs = probs, rank, alt_ids, alt_probs

    @classmethod
    def unpredicted(cls, n, k):
        """a text without a single prediction (n = 0 or 1 characters)"""
        return cls(np.ones(n, dtype=np.float32), np.full(n, -1, dtype=np.int32), np.full((n, k), -1, dtype=np.int32),
                   np.zeros((n, k), dtype=np.float32))

    def __len__(self):
        return len(self.probs)

    def chars(self, mapping):
        """the alternatives as characters, [n][k]: mapping is the Rater's (char -> id, id -> char) pair or its id -> char
        half; id 0 (the unmapped character) shows as the empty string, no alternative (-1) as None"""
        i_c = mapping[1] if isinstance(mapping, (tuple, list)) else mapping
        return [[None if v < 0 else i_c.get(int(v), "") for v in row] for row in self.alt_ids]


class Suspects(object):
    """One text's share of `Rater.suspects`, m suspect characters:

    positions  [m] i64    index into the normalised text, ascending
    probs      [m] f32    probability of the character written there
    rank       [m] i32    its position among all the model could have written there
    alt_ids    [m,k] i32  the k most probable ids there, most probable first (-1: none)
    alt_probs  [m,k] f32  their probabilities (0 where alt_ids is -1)
    """

    def __init__(self, positions, probs, rank, alt_ids, alt_probs):
        self.positions, self.probs, self.rank, self.alt_ids, self.alt_probs = positions, probs, rank, alt_ids, alt_probs

    def __len__(self):
        return len(self.positions)

    def chars(self, mapping):
        """the alternatives as characters, [m][k], as `RatedText.chars`"""
        return RatedText.chars(self, mapping)


class Corrections(Suspects):
    """One text's share of `Rater.corrections`: the m suspects of `Rater.suspects` (the five arrays above, bit for bit) and
    what rescoring their alternatives against the text that follows proposes.  With k alternatives and R = k + 1 (+ 1 with
    deletions, + k with insertions) variants per suspect -- 0: the character as written, v = 1 .. k: alt_ids[:, v-1] in its
    place, k + 1 (deletions): the character dropped, from k + 1 + deletions on (insertions): alt_ids[:, j] inserted in front
    of the character, j = 0 .. k-1 --:

    cost       [m,R] f64  bits of the variant's character(s) and the characters after it (+inf: no such variant)
    best_id    [m] i32    the id proposed in place of the character, or in front of it; NO_PROPOSAL (-1): none, DELETE (-2):
                          drop the character
    gain       [m] f64    bits saved by the proposal against the text as written (0.0 without a proposal)
    best_op    [m] i32    what the proposal does: OP_NONE, OP_SUBSTITUTE (best_id for the character), OP_DELETE, OP_INSERT
                          (best_id in front of the character, which stays); derived from best_id where it is not given
    """
    NO_PROPOSAL = -1
    DELETE = -2
    OP_NONE, OP_SUBSTITUTE, OP_DELETE, OP_INSERT = 0, 1, 2, 3

    def __init__(self, positions, probs, rank, alt_ids, alt_probs, cost, best_id, gain, best_op=None):
        Suspects.__init__(self, positions, probs, rank, alt_ids, alt_probs)
        self.cost, self.best_id, self.gain = cost, best_id, gain
        if best_op is None:
            ids = np.asarray(best_id)
            best_op = np.where(ids >= 0, self.OP_SUBSTITUTE, np.where(ids == self.DELETE, self.OP_DELETE, self.OP_NONE))
            best_op = best_op.astype(np.int32)
        self.best_op = best_op

    def proposals(self, mapping):
        """the proposals as characters, [m]: None for no proposal, "" for a deletion, else the character (substituted, or
        inserted: `best_op` says which, `edits` gives what replaces the written character) -- the unmapped id 0 has no
        character to write and shows as None too.  mapping as in `RatedText.chars`."""
        i_c = mapping[1] if isinstance(mapping, (tuple, list)) else mapping
        return ["" if v == self.DELETE else (i_c.get(int(v)) if v >= 0 else None) for v in self.best_id]

    def edits(self, text, mapping):
        """per suspect the string that replaces text[position], [m]: "" drops the character, "x" substitutes it, "xw" inserts
        x in front of the written w; None for no proposal, a proposal of the unmapped id 0 (no character to write) and a
        position outside the text.  text is the normalised text, mapping as in `RatedText.chars`."""
        out = []
        for at, op, new in zip(self.positions, self.best_op, self.proposals(mapping)):
            at = int(at)
            if new is None or op == self.OP_NONE or not 0 <= at < len(text):
                out.append(None)
            elif op == self.OP_INSERT:
                out.append(new + text[at])
            else:
                out.append(new)
        return out

    def apply(self, text, mapping):
        """the (normalised) text with the proposals applied (`edits`), from right to left so that positions stay true; a
        proposal of the unmapped id 0 leaves the character as written"""
        chars = list(text)
        edits = self.edits(text, mapping)
        for j in range(len(self.positions) - 1, -1, -1):
            if edits[j] is not None:
                at = int(self.positions[j])
                chars[at:at + 1] = list(edits[j])
        return "".join(chars)


class Rescored(object):
    """One text's share of `Rater.rescore`: its m spans in the order they were given and what rating the caller's candidates
    against the text around them proposes.  Span j is text[starts[j]:ends[j]] and owns candidates[first[j]:first[j + 1]]:

    starts, ends  [m] i64          the span in the normalised text (ends[j] == starts[j]: an insertion in front of starts[j])
    first         [m + 1] i64      where a span's candidates begin
    candidates    [first[m]] str   the (normalised) replacement strings, "" drops the span
    cost0         [m] f64          bits of the text as written over the span and the characters after it (+inf: the span has
                                   no prediction to be held against); None without want_costs
    cost          [first[m]] f64   the same with the candidate in place of the span (+inf: no such hypothesis); None without
                                   want_costs
    best          [m] i32          the index within the span's candidates of the one proposed, -1: none
    gain          [m] f64          bits saved by the proposal against the text as written (0.0 without a proposal)
    """

    def __init__(self, starts, ends, first, candidates, cost0, cost, best, gain):
        self.starts, self.ends, self.first, self.candidates = starts, ends, first, candidates
        self.cost0, self.cost, self.best, self.gain = cost0, cost, best, gain

    def __len__(self):
        return len(self.starts)

    def proposals(self):
        """per span the string proposed in its place, [m]: None for no proposal, "" for dropping the span"""
        return [None if b < 0 else self.candidates[int(a) + int(b)] for a, b in zip(self.first[:-1], self.best)]

    def apply(self, text):
        """the (normalised) text with the kept proposals written: they are taken in descending gain (ties: the earlier start,
        then the order given), one that overlaps a span already taken is skipped -- [a, b) and [c, d) overlap where a < d and
        c < b, and two insertions at the same place do --, and the taken ones are written from right to left so that
        positions stay true"""
        new = self.proposals()
        order = sorted((j for j in range(len(new)) if new[j] is not None),
                       key=lambda j: (-float(self.gain[j]), int(self.starts[j]), j))
        taken = []
        for j in order:
            a, b = int(self.starts[j]), int(self.ends[j])
            if not 0 <= a <= b <= len(text):
                continue
            if any((a < d and c < b) or (a == b == c == d) for c, d, _ in taken):
                continue
            taken.append((a, b, new[j]))
        chars = list(text)
        for a, b, string in sorted(taken, key=lambda e: (e[0], e[1]), reverse=True):
            chars[a:b] = list(string)
        return "".join(chars)


class ContextRating(object):
    """One text of `Rater.rate_contexts`, n characters rated under C candidate contexts:

    bits       [C] f64    bits of the text under every candidate, as `rate_batch(texts, contexts=candidates[c])` gives them
    posterior  [C] f64    the prior times 2**-bits, normalised: how much of the belief every candidate holds after the text
    best       int        the index into `candidates` of the most probable one (the smallest among equal ones)
    margin     float      bits between the best and the next candidate with a positive prior (+inf: there is no other)
    mix_bits   float      bits of the text under the sequential Bayesian mixture of the candidates
    probs      [n] f32    probability of every character under that mixture (1.0 for the first); None without want_probs
    """

    def __init__(self, bits, posterior, best, margin, mix_bits, probs):
        self.bits, self.posterior, self.best, self.margin = bits, posterior, int(best), float(margin)
        self.mix_bits, self.probs = float(mix_bits), probs

    def __len__(self):
        return len(self.bits)


class Words(object):
    """One text's share of `Rater.suspect_words`, m words in ascending order:

    start      [m] i64    position of the word in the normalised text
    length     [m] i32    its number of characters
    n          [m] i32    how many of them the model predicted (the text's first character has no prediction)
    bits       [m] f64    bits of the word: -sum log2(max(p, 1e-99)) over its predicted characters
    mean_prob  [m] f64    mean probability over the predicted characters (NaN where n is 0)
    min_prob   [m] f32    the least probability (+inf where n is 0)
    worst      [m] i64    position in the text of the least probable character, the first among equal ones (-1 where n is 0)
    suspects   [m] i32    how many of its characters are suspects (`Rater.suspects`' rule)
    """

    def __init__(self, start, length, n, bits, mean_prob, min_prob, worst, suspects):
        self.start, self.length, self.n, self.bits, self.mean_prob = start, length, n, bits, mean_prob
        self.min_prob, self.worst, self.suspects = min_prob, worst, suspects

    @classmethod
    def from_records(cls, start, end, n, bits, psum, least, worst, bad, offset=0):
        """from records in corpus positions (ratebulk.segments_host with their segments) of a text that begins at `offset` -- or
        of many texts, with one offset per record"""
        start, end, worst = (np.asarray(a, dtype=np.int64) for a in (start, end, worst))
        n = np.asarray(n, dtype=np.int32)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(n > 0, np.asarray(psum, dtype=np.float64) / np.maximum(n, 1), np.nan)
        return cls(start - offset, (end - start).astype(np.int32), n, np.asarray(bits, dtype=np.float64), mean,
                   np.asarray(least, dtype=np.float32), np.where(worst >= 0, worst - offset, -1), np.asarray(bad, dtype=np.int32))

    def __len__(self):
        return len(self.start)

    def cut(self, a, b):
        """the records a .. b - 1 as a result of their own"""
        return type(self)(*(f[a:b] for f in (self.start, self.length, self.n, self.bits, self.mean_prob, self.min_prob,
                                             self.worst, self.suspects)))

    def spans(self):
        """the words as [(start, end)] in the normalised text"""
        return [(int(a), int(a) + int(m)) for a, m in zip(self.start, self.length)]

    def strings(self, text):
        """the words as strings; text is the normalised text"""
        return [text[a:b] for a, b in self.spans()]


class Segments(Words):
    """One text's share of `Rater.rate_segments`: `Words`' fields for the caller's segments of that text, in the order given
    (`suspects` are zeros: no ranks are computed)."""


def word_edits(found, texts, candidates, priors=None):
    """Edits for `Rater.rescore` from the words `Rater.suspect_words` found: found is one `Words` per text, candidates a dict or
    a callable word -> list of replacement strings (a lexicon look-up, a spell checker, a second engine's token).  One edit
    (i, start, end, replacements) per word that yields replacements; a word that yields none is skipped, and so is a word at a
    text's first character (no prediction to be held against).  Ordered by text and start.  Host only.

    With priors -- a dict or a callable word -> one number per replacement of that word, e.g. a channel's bits -- returns
    (edits, prior): prior[e] is the list of numbers of edit e, parallel to its replacements: what `Rater.rescore(prior=..)`
    takes.  ValueError for a word whose numbers are not as many as its replacements."""
    if len(found) != len(texts):
        raise ValueError("word_edits: one Words per text")
    look_up = candidates if callable(candidates) else (lambda word: candidates.get(word, ()))
    weigh = None if priors is None else priors if callable(priors) else (lambda word: priors.get(word, ()))
    edits, prior = [], []
    for i, (words, text) in enumerate(zip(found, texts)):
        text = windows.normalize(text)
        for start, end in sorted(words.spans()):
            if start < 1:
                continue
            replacements = list(look_up(text[start:end]) or ())
            if replacements:
                edits.append((i, start, end, replacements))
                if weigh is not None:
                    prior.append([float(b) for b in weigh(text[start:end]) or ()])
                    if len(prior[-1]) != len(replacements):
                        raise ValueError("word_edits: one prior per replacement of %r" % text[start:end])
    return edits if weigh is None else (edits, prior)


def join_edits(found, texts, delimiter_of, joiner=" ", only=None):
    """Spans for `Rater.rescore` over PAIRS of words that a spurious `joiner` may have parted (`to gether`): found is one
    `Words` per text -- the selected words --, delimiter_of a callable character -> bool, the rater's delimiter table.  Per
    selected word (with `only`, a callable word -> bool: per selected word it accepts) the word before and the word after are
    looked at, if exactly one character separates them and that character is `joiner`; the neighbour's extent is found from the
    text, since `found` holds only selected words.  Returns [(i, start, end, joined)]: the span over the two words and the
    joiner in the normalised texts[i], and the two words run together -- what a look-up takes.  A pair is listed once, also
    where both of its words are selected; a span at a text's first character is skipped (no prediction to be held against),
    and so is a span of more than 64 characters (`rescore` takes no longer one).  Ordered by text, start and end.  Host only."""
    if len(found) != len(texts):
        raise ValueError("join_edits: one Words per text")
    joins = set()
    for i, (words, text) in enumerate(zip(found, texts)):
        text = windows.normalize(text)
        n = len(text)
        for a, b in words.spans():
            if only is not None and not only(text[a:b]):
                continue
            if a >= 2 and text[a - 1] == joiner and not delimiter_of(text[a - 2]):
                p = a - 2
                while p > 0 and not delimiter_of(text[p - 1]):
                    p -= 1
                joins.add((i, p, b, text[p:a - 1] + text[a:b]))
            if b + 1 < n and text[b] == joiner and not delimiter_of(text[b + 1]):
                e = b + 2
                while e < n and not delimiter_of(text[e]):
                    e += 1
                joins.add((i, a, e, text[a:b] + text[b + 1:e]))
    return sorted(j for j in joins if j[1] >= 1 and j[2] - j[1] <= ratebulk.SPAN_LEN_MAX)


class Lexicon(object):
    """A list of words to look suspect words up in (`Rater.lexicon` builds it, `Rater.lexicon_neighbours` and
    `Rater.correct_words` read it).  `entries` is an iterable of strings in priority order, the most frequent first; they are
    NFC-normalised and encoded with `mapping` (char -> id), ids below `voc_size`.  Dropped, and counted by reason in `dropped`
    ("empty", "long": more than 64 characters, "unmapped": a character outside the mapping, "duplicate": the first is kept):

    words        [N] str         the kept entries, in the order given -- what the neighbours' indices refer to
    pool, off    int32, int64 [N + 1]   their ids end to end and where each begins
    chars, order, class_first    the device layout of `ratebulk.lexicon_layout_host`
    mapping, voc_size            what it was encoded with
    dropped      dict            reason -> count
    """

    def __init__(self, entries, mapping, voc_size):
        if int(voc_size) > ratebulk.LEXICON_V_MAX:
            raise ValueError("a lexicon needs a mapping of at most %d characters (got %d)" % (ratebulk.LEXICON_V_MAX, voc_size))
        self.mapping, self.voc_size = mapping, int(voc_size)
        self._mapped = len(mapping)
        self.dropped = dict(empty=0, long=0, unmapped=0, duplicate=0)
        self.words = []
        seen = set()
        for entry in entries:
            word = windows.normalize(entry)
            reason = ("empty" if not word else "long" if len(word) > ratebulk.SPAN_LEN_MAX
                      else "unmapped" if any(not 0 < mapping.get(c, 0) < self.voc_size for c in word)
                      else "duplicate" if word in seen else None)
            if reason:
                self.dropped[reason] += 1
            else:
                seen.add(word)
                self.words.append(word)
        self.pool = windows.encode("".join(self.words), mapping).astype(np.int32)
        self.off = np.concatenate([[0], np.cumsum([len(w) for w in self.words])]).astype(np.int64)
        self.chars, self.order, self.class_first = ratebulk.lexicon_layout_host(self.pool, self.off)
        self._device = {}      # id(engine) -> (engine, chars, order) on its device: uploaded once

    def __len__(self):
        return len(self.words)

    def same_mapping(self, mapping):
        """was the lexicon encoded with this very mapping (the same object, no character added since)?"""
        return mapping is self.mapping and len(mapping) == self._mapped

    def on_device(self, lm):
        """(chars, order) as int32 tensors on the engine's device: uploaded at the first call, kept for the later ones"""
        held = self._device.get(id(lm))
        if held is None or held[0] is not lm:
            up = lambda a: lm.torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)
            held = self._device[id(lm)] = (lm, up(self.chars), up(self.order))
        return held[1], held[2]


class Neighbours(object):
    """What `Rater.lexicon_neighbours` returns for n words, in input order, K = per_word:

    exact   [n] i32     the index into `lexicon.words` of the word itself, -1: it is not in the lexicon
    found   [n] i32     how many entries lie within 1 .. max_dist edits of it, whatever K is
    index   [n,K] i32   the first K of them, ordered by (distance, index) -- the nearest first, the more frequent among equally
                        near ones --, -1 from the found-th on
    dist    [n,K] i32   their distances, -1 where index is
    bits    None, or with a channel [n,K] f64: dist then holds sixteenths of a bit under the channel -- `found` counts the entries
                        within max_bits --, bits their float value, NaN where index is -1
    """

    def __init__(self, lexicon, exact, found, index, dist, bits=None):
        self.lexicon, self.exact, self.found, self.index, self.dist, self.bits = lexicon, exact, found, index, dist, bits

    def __len__(self):
        return len(self.exact)

    def strings(self, i):
        """the neighbours of word i as strings, the nearest first"""
        return [self.lexicon.words[int(e)] for e in self.index[i] if e >= 0]


class Splits(object):
    """What `Rater.lexicon_splits` returns for n words, in input order, K = per_word:

    found   [n] i32     at how many places the word falls into two entries within max_dist edits, the lost delimiter being one
                        of them, whatever K is
    at      [n,K] i32   the first K of these places s -- word[:s] and word[s:] are the halves --, ordered by (dist, the larger of
                        the two indices, s): the nearest pair first, among equally near pairs the one whose rarer half is more
                        frequent; -1 from the found-th on
    left    [n,K] i32   the index into `lexicon.words` of the entry nearest to word[:s] (the more frequent among equally near ones)
    right   [n,K] i32   the same for word[s:]
    dist    [n,K] i32   1 + the two halves' distances; -1 where `at` is
    """

    def __init__(self, lexicon, found, at, left, right, dist):
        self.lexicon, self.found, self.at, self.left, self.right, self.dist = lexicon, found, at, left, right, dist

    def __len__(self):
        return len(self.found)

    def strings(self, i, joiner=" "):
        """the splits of word i as strings `left + joiner + right`, the nearest first"""
        words = self.lexicon.words
        return [words[int(a)] + joiner + words[int(b)] for a, b in zip(self.left[i], self.right[i]) if a >= 0]


class Chains(object):
    """What `Rater.lexicon_chains` returns for n words, in input order, P = max_parts:

    found   [n] i32       bit p-1 is set iff the word is a chain of exactly p entries (p = 1: the word is an entry itself), every
                          piece of at least min_part characters, a link allowed between neighbours
    worst   [n,P] i32     per p the chain's bottleneck: the largest index into `lexicon.words` among its pieces -- the rarest
                          part; the chain reported for a p is one of least bottleneck; -1 where there is none
    entry   [n,P,P] i32   entry[i, p-1, :p] the pieces of the chain of p parts, -1 behind them
    start   [n,P,P] i32   where each piece begins in the word
    link    [n,P,P] i32   link[i, p-1, k] the index into `links` of the link between piece k and k + 1, -1 for none
    links   [str]         the linking elements the call allowed, normalised
    """

    def __init__(self, lexicon, found, worst, entry, start, link, links=()):
        self.lexicon, self.found, self.worst, self.entry, self.start, self.link = lexicon, found, worst, entry, start, link
        self.links = list(links)

    def __len__(self):
        return len(self.found)

    def parts(self, i):
        """the least p for which word i is a chain of p entries, 0: it is none"""
        bits = int(self.found[i])
        return (bits & -bits).bit_length()

    def pieces(self, i, p):
        """the entries of word i's chain of p parts as strings, [] if there is none"""
        if not 1 <= p <= self.worst.shape[1] or not (int(self.found[i]) >> (p - 1)) & 1:
            return []
        return [self.lexicon.words[int(e)] for e in self.entry[i, p - 1, :p]]

    def strings(self, i, joiner=" ", min_parts=2):
        """one string per existing p >= min_parts, ascending: the pieces joined by `joiner`, a link attached to the piece
        in front of it"""
        out = []
        for p in range(max(1, int(min_parts)), self.worst.shape[1] + 1):
            pieces = self.pieces(i, p)
            if pieces:
                tails = [self.links[int(l)] if l >= 0 else "" for l in self.link[i, p - 1, :p - 1]] + [""]
                out.append(joiner.join(piece + tail for piece, tail in zip(pieces, tails)))
        return out


class Channel(object):
    """A table of confusions as the weighted look-up takes it (`Rater.channel` builds it, `Rater.lexicon_neighbours` and
    `Rater.correct_words` read it).  `records` is a `Confusions` or an iterable of (source, target, count, occ): `source` in
    the OCR stands for `target` in the truth, `count` times at `occ` occurrences of the source.  The strings are NFC-normalised
    and encoded with `mapping` (char -> id), ids below `voc_size`.  Costs are sixteenths of a bit: a record costs
    round(16 * min(-log2(count / occ), 255)), a plain edit `unit` = round(16 * unit_bits).  Dropped, and counted by reason in
    `dropped`: "count" and "rate" -- below min_count, below min_rate --, "empty" -- no source --, "same" -- the source is the
    target --, "unmapped" -- a character outside the mapping --, "long" -- a side of more than 4 characters --, "duplicate" -- the
    least cost of a (source, target) is kept --, "cut" -- beyond 1024 rules those of largest count are kept, the first among
    equal ones.

    sources, targets, count   [R]   the kept rules, in the order given
    rules    [R, 10] i32      src_len, tgt_len, src[4], tgt[4]: the records of kl_confusion_counts, as ids
    cost     [R] i32          sixteenths of a bit
    unit     int              the cost of a plain insertion, deletion or substitution
    mapping, voc_size         what it was encoded with
    dropped  dict             reason -> count
    """

    def __init__(self, records, mapping, voc_size, unit_bits=8.0, min_count=2, min_rate=0.0):
        if int(voc_size) > ratebulk.LEXICON_V_MAX:
            raise ValueError("a channel needs a mapping of at most %d characters (got %d)" % (ratebulk.LEXICON_V_MAX, voc_size))
        unit = int(round(ratebulk.CHANNEL_SCALE * float(unit_bits)))
        if not 1 <= unit <= ratebulk.CHANNEL_COST_MAX:
            raise ValueError("a channel's unit_bits lies in 1/16 .. 255.9 (got %r)" % (unit_bits,))
        self.mapping, self.voc_size, self.unit = mapping, int(voc_size), unit
        self._mapped = len(mapping)
        self.dropped = dict(count=0, rate=0, empty=0, same=0, unmapped=0, long=0, duplicate=0, cut=0)
        if isinstance(records, Confusions):
            records = zip(records.sources, records.targets, records.count.tolist(), records.occ.tolist())
        chars_max = ratebulk.CONFUSION_CHARS_MAX
        kept, place = [], {}
        for source, target, count, occ in records:
            source, target = windows.normalize(source), windows.normalize(target)
            count, occ = int(count), int(occ)
            rate = count / occ if occ > 0 else 0.0
            reason = ("count" if count < min_count else "rate" if rate < min_rate else "empty" if not source
                      else "same" if source == target else "long" if max(len(source), len(target)) > chars_max
                      else "unmapped" if any(not 0 < mapping.get(c, 0) < self.voc_size for c in source + target) else None)
            if reason:
                self.dropped[reason] += 1
                continue
            bits = 255.0 if rate <= 0.0 else min(max(-np.log2(rate), 0.0), 255.0)
            cost = int(round(ratebulk.CHANNEL_SCALE * bits))
            if (source, target) in place:
                self.dropped["duplicate"] += 1
                at = place[source, target]
                if cost < kept[at][3]:
                    kept[at] = (source, target, count, cost)
            else:
                place[source, target] = len(kept)
                kept.append((source, target, count, cost))
        if len(kept) > ratebulk.CHANNEL_RULES_MAX:
            first = sorted(range(len(kept)), key=lambda i: (-kept[i][2], i))[:ratebulk.CHANNEL_RULES_MAX]
            self.dropped["cut"] = len(kept) - len(first)
            kept = [kept[i] for i in sorted(first)]
        self.sources, self.targets = [r[0] for r in kept], [r[1] for r in kept]
        self.count = np.asarray([r[2] for r in kept], dtype=np.int64)
        self.cost = np.asarray([r[3] for r in kept], dtype=np.int32)
        self.rules = np.zeros((len(kept), 2 + 2 * chars_max), dtype=np.int32)
        for r, (source, target, _, _) in enumerate(kept):
            self.rules[r, 0], self.rules[r, 1] = len(source), len(target)
            self.rules[r, 2:2 + len(source)] = [mapping[c] for c in source]
            self.rules[r, 2 + chars_max:2 + chars_max + len(target)] = [mapping[c] for c in target]
        self._device = {}      # id(engine) -> (engine, rules, cost) on its device: uploaded once

    def __len__(self):
        return len(self.sources)

    def same_mapping(self, mapping):
        """was the channel encoded with this very mapping (the same object, no character added since)?"""
        return mapping is self.mapping and len(mapping) == self._mapped

    def on_device(self, lm):
        """(rules, cost) as int32 tensors on the engine's device, (None, None) for no rules: uploaded at the first call, kept
        for the later ones"""
        if not len(self):
            return None, None
        held = self._device.get(id(lm))
        if held is None or held[0] is not lm:
            up = lambda a: lm.torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)
            held = self._device[id(lm)] = (lm, up(self.rules), up(self.cost))
        return held[1], held[2]


class Alignment(object):
    """One pair of `Rater.align`, a text `a` against a witness `b` (both NFC-normalised):

    dist    int          the Levenshtein distance (unit costs) if it is at most max_dist; -1: more than max_dist edits apart --
                         not two readings of the same text; -2: a text longer than the call could take
    spans   [m, 4] i32   where they differ, ascending: a[a_start:a_end] reads b[b_start:b_end] in the witness (one side may be
                         empty: an insertion or a deletion); none for dist <= 0
    """

    def __init__(self, dist, spans):
        self.dist, self.spans = int(dist), spans

    def __len__(self):
        return len(self.spans)

    def strings(self, a, b):
        """the differences as [(written, witness_reading)]"""
        return [(a[a0:a1], b[b0:b1]) for a0, a1, b0, b1 in self.spans.tolist()]

    def apply(self, a, b):
        """a with every span replaced by the witness' reading, from right to left: the witness itself (where dist >= 0)"""
        chars = list(a)
        for a0, a1, b0, b1 in reversed(self.spans.tolist()):
            chars[a0:a1] = list(b[b0:b1])
        return "".join(chars)


def witness_edits(alignments, pairs, texts, witnesses, max_len=ratebulk.SPAN_LEN_MAX):
    """Edits for `Rater.rescore` from second readings of the texts: witnesses[i] is a sequence of strings (possibly none) that
    read the same line or page as texts[i], pairs[q] = (i, w) says that alignments[q] (`Rater.align`'s `Alignment`) is texts[i]
    against witnesses[i][w].  Returns (edits, skipped): one edit (i, start, end, readings) per differing span of a text, ordered
    by text and start; spans of one text with the same (start, end) from several witnesses pool their readings -- first seen
    first, duplicates dropped --, spans that merely overlap stay separate (`Rescored.apply` resolves overlaps by gain).
    `skipped` counts what yields no edit, by reason: "different" -- pairs with dist < 0 --, "first" -- spans with start == 0:
    no prediction to be held against, as `word_edits` skips them --, "long" -- spans with more than max_len characters on a
    side.  Host only."""
    if len(alignments) != len(pairs) or len(texts) != len(witnesses):
        raise ValueError("witness_edits: one alignment per pair, one sequence of witnesses per text")
    skipped = dict(different=0, first=0, long=0)
    pooled = {}
    for one, (i, w) in zip(alignments, pairs):
        if one.dist < 0:
            skipped["different"] += 1
            continue
        reading = windows.normalize(witnesses[i][w])
        for a0, a1, b0, b1 in one.spans.tolist():
            if a0 == 0:
                skipped["first"] += 1
            elif a1 - a0 > max_len or b1 - b0 > max_len:
                skipped["long"] += 1
            else:
                readings = pooled.setdefault((i, a0, a1), [])
                if reading[b0:b1] not in readings:
                    readings.append(reading[b0:b1])
    return [(i, a0, a1, pooled[i, a0, a1]) for i, a0, a1 in sorted(pooled)], skipped


class Consensus(Rescored):
    """One text's share of `Rater.consensus`: a `Rescored` whose m spans are the clusters of its witnesses' differences, ascending,
    and whose candidates are the witnesses' distinct readings of a whole cluster, in order of the first witness that gives one.
    cost0 and cost are SCORES: the reading's bits minus vote_bits per vote (with vote_bits = 0.0 the model's bits alone); `gain`
    is the score of the text as written minus the best score.  In addition:

    votes0   [m] i32          1 (the text itself) plus the accepted witnesses that agree with the text over the span
    votes    [first[m]] i32   the accepted witnesses that read the candidate; a span's votes sum to 1 plus the text's accepted
                              witnesses
    """

    def __init__(self, starts, ends, first, candidates, cost0, cost, best, gain, votes0, votes):
        Rescored.__init__(self, starts, ends, first, candidates, cost0, cost, best, gain)
        self.votes0, self.votes = votes0, votes


class Confusions(object):
    """What `Rater.confusions` returns: the table of confusions of OCR texts held against their ground truth.

    sources, targets   [R] str   record i: `sources[i]` in the OCR stands for `targets[i]` in the truth ("" for characters the
                                 OCR added; never an empty source: lost characters are anchored on a neighbour), in order of
                                 first occurrence
    count     [R] i64            the spans that gave the record
    occ       [R] i64            how often its source stands in the OCR texts of the accepted pairs, overlaps included
    dist      [P] i32            per pair, as `Alignment.dist`
    chars, edits, cer            truth characters of the accepted pairs (dist >= 0), the sum of their dist, and edits / chars
                                 (0.0 for no characters): the character error rate
    skipped   dict               what gave no record: "different" -- pairs with dist < 0 --, "long" -- spans with more than
                                 max_chars characters on a side --, "empty" -- spans of an empty OCR text
    spans     int                the spans that gave a record (the sum of count)
    """

    def __init__(self, rules, count, occ, stats, dist, truth_sizes):
        rules = np.asarray(rules, dtype=np.int32).reshape(-1, 2 + 2 * ratebulk.CONFUSION_CHARS_MAX)
        word = lambda symbols: "".join(chr(int(c)) for c in symbols)
        self.sources = [word(r[2:2 + r[0]]) for r in rules]
        self.targets = [word(r[2 + ratebulk.CONFUSION_CHARS_MAX:2 + ratebulk.CONFUSION_CHARS_MAX + r[1]]) for r in rules]
        self.count, self.occ = np.asarray(count, dtype=np.int64), np.asarray(occ, dtype=np.int64)
        self.dist = np.asarray(dist, dtype=np.int32)
        accepted = self.dist >= 0
        self.chars = int(np.asarray(truth_sizes, dtype=np.int64)[accepted].sum())
        self.edits = int(self.dist[accepted].sum())
        self.cer = self.edits / self.chars if self.chars else 0.0
        self.spans = int(stats[1])
        self.skipped = dict(different=int((~accepted).sum()), long=int(stats[2]), empty=int(stats[3]))

    def __len__(self):
        return len(self.sources)

    def rate(self, i):
        """the share of its source's occurrences at which record i was read"""
        return float(self.count[i]) / float(self.occ[i]) if self.occ[i] else 0.0

    def kept(self, min_count=2, min_rate=0.0, per_source=3):
        """the records `rules` keeps, as [[indices of one source]]: records below min_count or min_rate dropped, those of a
        source ordered by (-count, first occurrence) and cut to per_source, the sources by their best record likewise"""
        by_source = {}
        for i in range(len(self)):
            if self.count[i] >= min_count and self.rate(i) >= min_rate:
                by_source.setdefault(self.sources[i], []).append(i)
        order = lambda i: (-int(self.count[i]), i)
        groups = [sorted(rows, key=order)[:max(int(per_source), 0)] for rows in by_source.values()]
        return sorted([rows for rows in groups if rows], key=lambda rows: order(rows[0]))

    def rules(self, min_count=2, min_rate=0.0, per_source=3):
        """[(source, [replacements])] as `confusion_edits` and `keraslm-rate rescore --confusions` take them ("" drops the
        source): see `kept`"""
        return [(self.sources[rows[0]], [self.targets[i] for i in rows]) for rows in self.kept(min_count, min_rate, per_source)]

    def write(self, file, **same):
        """`rules(**same)` as the TSV that `keraslm-rate rescore --confusions` reads -- a source, then its replacements, separated
        by tabs -- to a path or an open text file.  A tab or a line break cannot be written: replacements that hold one are left
        out, and so is a source that holds one or keeps no replacement.  Returns the number of lines."""
        unwritable = lambda word: any(c in word for c in "\t\n\r")
        lines = []
        for source, replacements in self.rules(**same):
            replacements = [r for r in replacements if not unwritable(r)]
            if replacements and not unwritable(source):
                lines.append("\t".join([source] + replacements) + "\n")
        if hasattr(file, "write"):
            file.write("".join(lines))
        else:
            with open(file, mode="w") as out:
                out.write("".join(lines))
        return len(lines)


def confusion_edits(texts, rules, at=None):
    """Edits for `Rater.rescore` from a table of known confusions: rules is a list of (source, [replacements]) with a non-empty
    source; one edit (i, start, end, replacements) per occurrence of a source in the NFC-normalised texts[i], overlapping
    occurrences included, ordered by text, start and rule.  Sources and replacements are normalised too; "" among the
    replacements drops the source.  With `at` (per text an array of positions, e.g. `Suspects.positions`) only occurrences whose
    span holds one of these positions are kept.  Host only."""
    rules = [(windows.normalize(source), [windows.normalize(r) for r in replacements]) for source, replacements in rules]
    if any(not source for source, _ in rules):
        raise ValueError("confusion_edits: a rule needs a non-empty source")
    if at is not None and len(at) != len(texts):
        raise ValueError("confusion_edits: one array of positions per text")
    edits = []
    for i, text in enumerate(texts):
        text = windows.normalize(text)
        marks = None if at is None else np.sort(np.asarray(at[i], dtype=np.int64).reshape(-1))
        here = []
        for n, (source, replacements) in enumerate(rules):
            start = text.find(source)
            while start >= 0:
                end = start + len(source)
                if marks is None or np.searchsorted(marks, start, side="left") < np.searchsorted(marks, end, side="left"):
                    here.append((start, n, end, replacements))
                start = text.find(source, start + 1)
        edits += [(i, start, end, list(replacements)) for start, n, end, replacements in sorted(here, key=lambda e: e[:2])]
    return edits


def alternatives_of(full, y, k):
    """What the model expected instead, from whole distributions: full [B,T,V] (probabilities, or logits -- any values that
    order the vocabulary), y [B,T] targets, k >= 1.  Within a position the ids are ordered by (value descending, id
    ascending) -- a stable sort, so exact ties resolve to the lower id.  Returns
      tprob  [B,T]    full[b,t,y], 0 where y is no id (y < 0 or y >= V), dtype of `full`
      alt_id [B,T,k]  int32: the first k ids in that order, -1 from the V-th on
      alt_p  [B,T,k]  their values in `full`, 0 where alt_id is -1
      rank   [B,T]    int32: the position of y in the order (0: the first choice; a tied target is counted by id), -1 where
                      y is no id.
    A position with y < 0 (padded tail, dummy stream) delivers nothing: 0, -1, 0, -1.  This is the numpy statement of what
    kl_rate_window_alts computes on the device."""
    full = np.asarray(full)
    y = np.asarray(y)
    B, T, V = full.shape
    k = int(k)
    m = min(k, V)
    order = np.argsort(-full, axis=2, kind="stable")
    alt_id = np.full((B, T, k), -1, dtype=np.int32)
    alt_p = np.zeros((B, T, k), dtype=full.dtype)
    alt_id[:, :, :m] = order[:, :, :m]
    alt_p[:, :, :m] = np.take_along_axis(full, order[:, :, :m], axis=2)
    known = (y >= 0) & (y < V)
    at = np.where(known, y, 0)
    fy = np.take_along_axis(full, at[:, :, None], axis=2)
    ahead = (full > fy) | ((full == fy) & (np.arange(V)[None, None, :] < at[:, :, None]))
    rank = np.where(known, ahead.sum(axis=2), -1).astype(np.int32)
    tprob = np.where(known, fy[:, :, 0], 0).astype(full.dtype)
    none = y < 0
    alt_id[none] = -1
    alt_p[none] = 0
    return tprob, alt_id, alt_p, rank


def plan(ids, contexts, length, streams):
    """ids: one int32 id vector per text (`windows.encode`); contexts: one (clamped) context list per text;
    length: window length T; streams: upper limit of rows.  Returns a Plan, or None if no text has a window."""
    n = len(ids)
    T = int(length)
    sizes = np.array([len(a) for a in ids], dtype=np.int64)
    count = np.array([windows.count_windows(int(s), T) for s in sizes], dtype=np.int64)
    n_ctx = len(contexts[0]) if n else 0
    total = int(count.sum())
    if total == 0:
        return None
    B = int(min(max(1, int(streams)), int((count > 0).sum())))
    # every window of every text, padded as stateful_windows pads the last one (x 0, ctx 0, y -1), plus one idle window
    X = np.zeros((total + 1) * T, dtype=np.int32)
    Y = np.full((total + 1) * T, -1, dtype=np.int32)
    C = np.zeros((total + 1, n_ctx), dtype=np.int32)
    offset = np.concatenate([[0], np.cumsum(count)])[:-1]
    for i in range(n):
        if count[i]:
            a, m = int(offset[i]) * T, int(sizes[i]) - 1
            X[a:a + m] = ids[i][:-1]
            Y[a:a + m] = ids[i][1:]
            C[offset[i]:offset[i] + count[i]] = np.asarray(contexts[i], dtype=np.int32)
    X, Y = X.reshape(total + 1, T), Y.reshape(total + 1, T)
    Z = (Y >= 0)[:, :, None].astype(np.int32) * C[:, None, :]
    # list scheduling, longest first: the next text goes to the row that is free first
    order = [int(i) for i in np.argsort(-count, kind="stable") if count[i] > 0]
    free = np.zeros(B, dtype=np.int64)
    row = np.full(n, -1, dtype=np.int64)
    first = np.zeros(n, dtype=np.int64)
    for i in order:
        r = int(np.argmin(free))
        row[i], first[i] = r, free[r]
        free[r] += count[i]
    n_calls = int(free.max())
    slots = np.full((n_calls, B), total, dtype=np.int64)       # (total: the idle window)
    for i in order:
        slots[first[i]:first[i] + count[i], row[i]] = np.arange(offset[i], offset[i] + count[i])
    return Plan(B, T, n_calls, row, first, count, sizes, X, Y, Z, slots)


def bits_of(probs):
    """-sum log2(max(p, 1e-99)) over all but the first character (the clamp of rating.py:531-576)"""
    p = np.asarray(probs, dtype=np.float64)[1:]
    return float(-np.log2(np.maximum(p, 1e-99)).sum()) if len(p) else 0.0
