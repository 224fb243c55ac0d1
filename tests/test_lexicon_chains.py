"""Lexicon chains on the CPU: `ratebulk.lexicon_chains_host`, `ratebatch.Chains`, `Rater.lexicon_chains`,
`Rater.correct_words(compounds=.., links=.., max_parts=..)` and `keraslm-rate lexicon --compounds --links --max-parts`.

The numpy statement of kl_lexicon_chains is held to a brute-force enumeration of all chains; the device kernel is held to the
statement in test_lexicon_chains_gpu.py.  The oracle-backed engine double has no `lexicon_chains`, so the Rater runs the
statement -- the chain around it is the product's, and is held to the same chain written out by hand."""
import json
import re

import numpy as np
import pytest
from click.testing import CliRunner

from oracle import lstm_oracle as O
from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.oracle_engine import OracleLM
from tests.test_lexicon import pooled, same_rescored
from tests.test_lexicon_splits import RESCORING, RULE

LENGTH = 16
ALPHABET = "abefhimnorstu \n"      # (what `arbeitsamt`, `bahnhof` and `inthehouse` need)


# ---------------------------------------------------------------------------------------------- the numpy statement
def same_id(x, y, V):
    return x == y and 0 <= x < V


def brute_chains(query, entries, V, links, P, min_part):
    """all chains of the query by enumeration: {p: the least bottleneck of a chain of p parts}"""
    m = len(query)
    least = {}
    if not max(1, min_part) <= m <= 64:
        return least

    def piece(a, b):
        for e, entry in enumerate(entries):
            if len(entry) == b - a and all(same_id(x, y, V) for x, y in zip(query[a:b], entry)):
                return e
        return None

    def walk(a, parts, worst):
        for b in range(a + min_part, m + 1):
            e = piece(a, b)
            if e is None:
                continue
            key = max(worst, e)
            if b == m:
                least[parts + 1] = min(least.get(parts + 1, key), key)
            elif parts + 1 < P:
                walk(b, parts + 1, key)
                for one in links:
                    if b + len(one) < m and all(same_id(x, y, V) for x, y in zip(query[b:b + len(one)], one)):
                        walk(b + len(one), parts + 1, key)

    walk(0, 0, -1)
    return least


def valid_chain(query, entries, V, links, min_part, p, entry, start, link):
    """the row (entry, start, link) of p parts is a chain of the query; returns its bottleneck"""
    assert (entry[p:] == -1).all() and (start[p:] == -1).all() and (link[max(p - 1, 0):] == -1).all()
    assert start[0] == 0 and (entry[:p] >= 0).all()
    at = 0
    for k in range(p):
        e = entries[entry[k]]
        assert start[k] == at and len(e) >= min_part
        assert len(query[at:at + len(e)]) == len(e) and all(same_id(x, y, V) for x, y in zip(query[at:at + len(e)], e))
        # the smallest index of the identical entries
        assert all(len(o) != len(e) or not all(same_id(x, y, V) for x, y in zip(o, e)) for o in entries[:entry[k]])
        at += len(e)
        if k < p - 1 and link[k] >= 0:
            one = links[link[k]]
            assert all(same_id(x, y, V) for x, y in zip(query[at:at + len(one)], one)) and at + len(one) < len(query)
            at += len(one)
    assert at == len(query)
    return int(entry[:p].max())


def test_lexicon_chains_host_against_all_chains():
    rng = np.random.default_rng(40)
    seen_p, n_links_used, n_rows = set(), 0, 0
    for trial in range(400):
        V = int(rng.integers(2, 4))
        odd = trial % 7 == 0      # (ids outside [0, V) among the entries and the queries)
        entries = [rng.integers(-1 if odd else 0, V + odd, int(rng.integers(1, 5))).tolist() for _ in range(int(rng.integers(1, 26)))]
        links = [rng.integers(0, V, int(rng.integers(1, 4))).tolist() for _ in range(int(rng.integers(0, 3)))]
        P, min_part = int(rng.integers(2, 6)), int(rng.integers(1, 3))
        queries = [rng.integers(-1 if odd else 0, V + odd, int(rng.integers(0, 11))).tolist() for _ in range(3)]
        # entries run together, a link between some
        parts = [entries[int(i)] for i in rng.integers(0, len(entries), int(rng.integers(1, 5)))]
        queries.append([i for k, e in enumerate(parts) for i in (e + (links[0] if links and k % 2 == 0 and k + 1 < len(parts) else []))][:10])
        layout = ratebulk.lexicon_layout_host(*pooled(entries))
        found, worst, entry, start, link = ratebulk.lexicon_chains_host(*pooled(queries), *layout, V, links, P, min_part)
        assert [a.dtype for a in (found, worst, entry, start, link)] == [np.int32] * 5
        assert worst.shape == (len(queries), P) and entry.shape == start.shape == link.shape == (len(queries), P, P)
        for q, query in enumerate(queries):
            want = brute_chains(query, entries, V, links, P, min_part)
            assert found[q] == sum(1 << (p - 1) for p in want), (trial, q)
            for p in range(1, P + 1):
                if p in want:
                    assert worst[q, p - 1] == want[p], (trial, q, p)
                    assert valid_chain(query, entries, V, links, min_part, p, entry[q, p - 1], start[q, p - 1], link[q, p - 1]) == want[p]
                    seen_p.add(p)
                    n_rows += 1
                    n_links_used += int((link[q, p - 1] >= 0).sum())
                else:
                    assert worst[q, p - 1] == -1 and (entry[q, p - 1] == -1).all() and (start[q, p - 1] == -1).all()
                    assert (link[q, p - 1] == -1).all()
    assert seen_p == {1, 2, 3, 4, 5} and n_links_used > 20 and n_rows > 400


def ids(word):
    return [ord(c) - ord("a") for c in word]


def chains_of(words, entries, links=(), P=4, min_part=1, V=26):
    as_ids = lambda w: w if isinstance(w, list) else ids(w)
    layout = ratebulk.lexicon_layout_host(*pooled([as_ids(e) for e in entries]))
    return ratebulk.lexicon_chains_host(*pooled([as_ids(w) for w in words]), *layout, V, [as_ids(l) for l in links], P, min_part)


def test_hand_made_chains():
    # `abababab` over ab, abab, ..: one row per p, the tie at p = 3 goes to the longest last piece
    found, worst, entry, start, link = chains_of([[0, 1] * 4], [[0, 1] * n for n in range(1, 6)], V=4)
    assert found.tolist() == [0b1111] and worst[0].tolist() == [3, 1, 1, 0]
    assert entry[0].tolist() == [[3, -1, -1, -1], [1, 1, -1, -1], [0, 0, 1, -1], [0, 0, 0, 0]]
    assert start[0].tolist() == [[0, -1, -1, -1], [0, 4, -1, -1], [0, 2, 4, -1], [0, 2, 4, 6]] and (link == -1).all()
    # a compound with a link, and the link's places: not at the ends, not counted by min_part
    entries = ["arbeit", "amt", "s", "dampf", "schiff", "fahrt", "in", "the", "house"]
    found, worst, entry, start, link = chains_of(["arbeitsamt", "dampfschiffahrt", "inthehouse", "arbeitamts", "sarbeitamt", "amt"],
                                                 entries, links=["s"], P=3, min_part=2)
    assert found.tolist() == [0b010, 0, 0b100, 0, 0, 0b001]      # (`schiffahrt` holds no `fahrt` behind `schiff`)
    assert entry[0, 1].tolist() == [0, 1, -1] and start[0, 1].tolist() == [0, 7, -1] and link[0, 1].tolist() == [0, -1, -1]
    assert entry[2, 2].tolist() == [6, 7, 8] and start[2, 2].tolist() == [0, 2, 5] and link[2, 2].tolist() == [-1, -1, -1]
    # with min_part 1 `s` is a piece: three parts, no link; two parts through the link
    found, worst, entry, start, link = chains_of(["arbeitsamt"], entries, links=["s"], P=3, min_part=1)
    assert found.tolist() == [0b110] and entry[0, 2].tolist() == [0, 2, 1] and link[0, 1, 0] == 0 and link[0, 2].tolist() == [-1, -1, -1]
    # `arbeits` an entry too: the bottleneck decides; on equal keys the no-link chain (visited first) is kept
    for lexicon, want_entry, want_link in ((["arbeits", "arbeit", "amt"], [0, 2], -1), (["arbeit", "amt", "arbeits"], [0, 1], 0),
                                           (["amt", "arbeit", "arbeits"], [1, 0], 0), (["arbeit", "arbeits", "amt"], [1, 2], -1)):
        found, worst, entry, start, link = chains_of(["arbeitsamt"], lexicon, links=["s"], P=2, min_part=2)
        assert found.tolist() == [0b10] and entry[0, 1].tolist() == want_entry and link[0, 1, 0] == want_link, lexicon
    # two identical links: the smaller index; links of 2 and 3 ids
    found, worst, entry, start, link = chains_of(["abxcd", "abxycd", "abxyzcd", "abxyzwcd"], ["ab", "cd"], links=["x", "x", "xy", "xyz"], P=2)
    assert found.tolist() == [2, 2, 2, 0] and link[:3, 1, 0].tolist() == [0, 2, 3]
    # queries that are no chain at all
    found, worst, entry, start, link = chains_of(["", "ab" * 33, "a"], ["ab", "a"], P=2, min_part=2)
    assert found.tolist() == [0, 0, 0] and (worst == -1).all() and (entry == -1).all()
    assert chains_of(["ab" * 32], ["ab" * 4], P=8, min_part=8)[0].tolist() == [0b10000000]
    assert chains_of(["ab" * 32], ["ab" * 4, "ab" * 2], P=8, min_part=8)[0].tolist() == [0b10000000]
    # ids outside [0, V) equal nothing, themselves included
    assert chains_of([[26, 1, 0, 1], [0, 1, 0, 1]], [[26, 1], [0, 1]], P=2)[0].tolist() == [0, 2]
    for wrong in (dict(P=1), dict(P=9), dict(min_part=0), dict(min_part=33), dict(V=0), dict(links=[""]), dict(links=["abcd"]),
                  dict(links=["a"] * 9), dict(links=[[26]]), dict(links=[[-1]])):
        with pytest.raises(ValueError):
            chains_of(["abab"], ["ab"], **wrong)


# ---------------------------------------------------------------------------------------------- the Rater on the double
def chain_rater(factory, length=LENGTH, seed=7):
    """test_rate_bulk_gpu.small_rater over the letters of `arbeitsamt` and `inthehouse`"""
    from ocrd_keraslm_amd.lib import Rater
    r = Rater(engine_factory=factory) if factory is not None else Rater()
    r.width, r.depth, r.length = 64, 2, length
    r.stateful = True
    r.mapping = (dict((c, i) for i, c in enumerate(sorted(ALPHABET), 1)), dict((i, c) for i, c in enumerate(sorted(ALPHABET), 1)))
    r.voc_size = len(ALPHABET) + 1
    r.configure()
    cfg = O.ModelConfig(2, 64, r.voc_size, 1)
    r.model.set_weights(O.init_weights(cfg, seed=seed, emb_std=0.3, dtype=np.float32), 3)
    r.status = 2
    return r


ENTRIES = ["the", "in", "a", "it", "house", "arbeit", "amt", "out", "he", "bahn", "hof", "ohne", "use", "reise", "on"]
TEXTS = ["a arbeitsamt inthehouse it", "in bahnhof\nouttheamt reisebahnhof a", "", "he inthe hause arbeitamt on",
         "it arbeitsamthof the inahouse"]


def encoded(r, strings):
    return pooled([[r.mapping[0].get(c, 0) for c in w] for w in strings])


def test_rater_lexicon_chains_on_the_double():
    r = chain_rater(OracleLM)
    lex = r.lexicon(ENTRIES)
    words = ["arbeitsamt", "inthehouse", "bahnhof", "house", "", "arbeitsamt", "reisebahnhof", "in?house", "ab" * 40, "hause", "inahouse"]
    chains = r.lexicon_chains(iter(words), lex, max_parts=3, min_part=2, links=("s",))
    assert type(chains) is ratebatch.Chains and len(chains) == len(words) and chains.links == ["s"]
    want = ratebulk.lexicon_chains_host(*encoded(r, words), lex.chars, lex.order, lex.class_first, r.voc_size,
                                        [[r.mapping[0]["s"]]], 3, 2)
    for got, ref in zip((chains.found, chains.worst, chains.entry, chains.start, chains.link), want):
        assert got.dtype == np.int32 and np.array_equal(got, ref)
    assert chains.found.tolist() == [0b010, 0b100, 0b010, 0b001, 0, 0b010, 0b100, 0, 0, 0, 0]
    assert [chains.parts(i) for i in range(len(words))] == [2, 3, 2, 1, 0, 2, 3, 0, 0, 0, 0]
    assert chains.pieces(0, 2) == ["arbeit", "amt"] and chains.pieces(0, 3) == [] and chains.pieces(3, 1) == ["house"]
    assert chains.strings(0) == ["arbeits amt"] and chains.strings(1) == ["in the house"] and chains.strings(1, "\n") == ["in\nthe\nhouse"]
    assert chains.strings(2, min_parts=3) == [] and chains.strings(3) == [] and chains.strings(3, min_parts=1) == ["house"]
    assert chains.worst[1].tolist() == [-1, -1, 4] and chains.start[6, 2].tolist() == [0, 5, 9]
    # min_part 1 lets `a` in; several rows of one word, ascending
    more = r.lexicon_chains(["inahouse", "inthehouse"], lex, max_parts=4, min_part=1)
    assert more.strings(0) == ["in a house"] and more.strings(1) == ["in the house"] and more.links == []
    none = r.lexicon_chains([], lex, max_parts=5)
    assert len(none) == 0 and none.worst.shape == (0, 5) and none.entry.shape == (0, 5, 5) and none.found.dtype == np.int32
    none = r.lexicon_chains(["inthehouse"], r.lexicon([""]), max_parts=2)
    assert none.found.tolist() == [0] and (none.worst == -1).all() and (none.entry == -1).all() and none.link.shape == (1, 2, 2)
    for wrong in (dict(max_parts=1), dict(max_parts=9), dict(min_part=0), dict(min_part=33), dict(links=["s"] * 9), dict(links=[""]),
                  dict(links=["stst"]), dict(links=["x"]), dict(links=["s", "?"])):
        with pytest.raises(ValueError):
            r.lexicon_chains(["inthehouse"], lex, **wrong)
    with pytest.raises(ValueError):
        r.lexicon_chains(["inthehouse"], ENTRIES)
    with pytest.raises(ValueError):
        r.lexicon_chains(["inthehouse"], chain_rater(OracleLM).lexicon(ENTRIES))      # another mapping object


def chain_by_hand(r, texts, contexts, lex, max_dist, per_word, known, min_part, compounds, links, max_parts, rule, rescoring,
                  joiner=" "):
    """correct_words(boundaries=True, compounds=.., links=.., max_parts=..) written out: suspect_words, the look-ups through
    the host statements, the candidates and the pairs found here from the texts themselves, rescore"""
    found, bits = r.suspect_words(texts, contexts, **rule)
    layout = (lex.chars, lex.order, lex.class_first, r.voc_size)
    words = sorted(set(w for one, t in zip(found, texts) for w in one.strings(t)))
    exact, _, cand, _ = ratebulk.lexicon_neighbours_host(*encoded(r, words), *layout, max_dist, per_word)
    as_entry = dict((w, bool(exact[q] >= 0)) for q, w in enumerate(words))
    unknown = [w for w in words if not as_entry[w]]
    if compounds and unknown:
        link_ids = [[r.mapping[0][c] for c in one] for one in links]
        bits_of = ratebulk.lexicon_chains_host(*encoded(r, unknown), *layout, link_ids, compounds, min_part)[0]
        for q, w in enumerate(unknown):
            as_entry[w] = bool(bits_of[q] >> 1)
    looked = dict((w, bool(known or not as_entry[w])) for w in words)
    table = dict((w, [lex.words[i] for i in cand[q] if i >= 0] if looked[w] else []) for q, w in enumerate(words))
    apart = [w for w in words if looked[w] and len(w) < 64]
    if apart:
        _, _, left, right, _ = ratebulk.lexicon_splits_host(*encoded(r, apart), *layout, max_dist, min_part, per_word)
        rows = ratebulk.lexicon_chains_host(*encoded(r, apart), *layout, [], max_parts, min_part) if max_parts >= 3 else None
        for q, w in enumerate(apart):
            strings = [lex.words[a] + joiner + lex.words[b] for a, b in zip(left[q], right[q]) if a >= 0]
            for p in range(3, max_parts + 1):
                if rows is not None and (rows[0][q] >> (p - 1)) & 1:
                    strings.append(joiner.join(lex.words[e] for e in rows[2][q, p - 1, :p]))
            for string in strings:
                if string not in table[w] and len(string) <= 64:
                    table[w].append(string)
    edits = ratebatch.word_edits(found, texts, table)
    pairs = []
    for i, (one, text) in enumerate(zip(found, texts)):
        chosen = set(one.spans())
        tokens = [(t.start(), t.end()) for t in re.finditer(r"[^ \n]+", text)]
        for (a, b), (c, e) in zip(tokens, tokens[1:]):
            mine = ((a, b) in chosen and looked[text[a:b]]) or ((c, e) in chosen and looked[text[c:e]])
            if c == b + 1 and text[b] == joiner and mine and a >= 1 and e - a <= 64:
                pairs.append((i, a, e, text[a:b] + text[c:e]))
    if pairs:
        exact, _, cand, _ = ratebulk.lexicon_neighbours_host(*encoded(r, [p[3] for p in pairs]), *layout, max_dist - 1, per_word)
        for q, (i, a, e, _) in enumerate(pairs):
            strings = [lex.words[j] for j in [exact[q]] + cand[q].tolist() if j >= 0]
            if strings:
                edits.append((i, a, e, strings))
    edits.sort(key=lambda e: e[:3])
    return found, edits, r.rescore(texts, edits, contexts, **rescoring), bits


def test_correct_words_with_compounds_and_longer_splits_is_the_chain_by_hand():
    r = chain_rater(OracleLM)
    lex = r.lexicon(ENTRIES)
    contexts = [[170 + i] for i in range(len(TEXTS))]
    by_case = {}
    for known, max_dist, min_part, compounds, links, max_parts in ((False, 2, 2, 0, (), 3), (False, 2, 2, 3, ("s",), 3),
                                                                   (False, 1, 2, 2, ("s", "es"), 3), (True, 2, 1, 3, ("s",), 4),
                                                                   (False, 2, 2, 3, (), 2)):
        found, rescored, bits = r.correct_words(TEXTS, lex, contexts, max_dist=max_dist, per_word=4, known=known, boundaries=True,
                                                min_part=min_part, compounds=compounds, links=links, max_parts=max_parts,
                                                **dict(RULE, **RESCORING))
        ref_found, edits, ref_rescored, ref_bits = chain_by_hand(r, TEXTS, contexts, lex, max_dist, 4, known, min_part, compounds,
                                                                 links, max_parts, RULE, RESCORING)
        assert np.array_equal(bits, ref_bits) and [one.spans() for one in found] == [one.spans() for one in ref_found]
        same_rescored(rescored, ref_rescored)
        assert sum(len(one) for one in rescored) == len(edits) > 0
        by_case[compounds, links, max_parts] = dict(((i, a, b), c) for i, a, b, c in edits)
    # `inthehouse` (text 0, 13 .. 23) falls into three entries only with max_parts >= 3
    assert "in the house" in by_case[0, (), 3][0, 13, 23] and "in the house" not in by_case[3, (), 2].get((0, 13, 23), [])
    assert "out the amt" in by_case[0, (), 3][1, 11, 20]
    # `arbeitsamt` (text 0, 2 .. 12): without compounds the split `arbeit amt` is offered, as a compound it is left alone;
    # `bahnhof` needs no link, `arbeitsamt` does
    assert "arbeit amt" in by_case[0, (), 3][0, 2, 12] and (0, 2, 12) not in by_case[3, ("s",), 3]
    assert (0, 2, 12) in by_case[3, (), 2] and (1, 3, 10) not in by_case[3, (), 2] and (1, 3, 10) in by_case[0, (), 3]
    # a chain of three parts is no compound of two
    assert (1, 21, 33) not in by_case[3, ("s",), 3] and "reise bahn hof" in by_case[2, ("s", "es"), 3][1, 21, 33]
    # with known=True a compound is looked up as an entry is
    assert (0, 2, 12) in by_case[3, ("s",), 4] and "in a house" in by_case[3, ("s",), 4][4, 21, 29]


def test_correct_words_with_longer_splits_and_a_channel():
    """a chain of p parts costs channel_weight * unit_bits * (p - 1), behind the pairs' unit_bits * dist"""
    r = chain_rater(OracleLM)
    lex = r.lexicon(ENTRIES)
    channel = r.channel([("a", "e", 30, 100)], unit_bits=4.0)
    contexts = [[170 + i] for i in range(len(TEXTS))]
    seen = {}
    real = r.rescore
    r.rescore = lambda texts, edits, contexts=None, **more: seen.update(edits=list(edits), prior=more.get("prior")) or real(texts, edits, contexts, **more)
    r.correct_words(TEXTS, lex, contexts, max_dist=2, per_word=4, boundaries=True, max_parts=3, channel=channel, max_bits=9.0,
                    channel_weight=0.5, **dict(RULE, **RESCORING))
    by_span = dict((e[:3], (e[3], p)) for e, p in zip(seen["edits"], seen["prior"]))
    assert all(len(p) == len(e[3]) for p, e in zip(seen["prior"], seen["edits"]))
    strings, weights = by_span[0, 13, 23]
    assert weights[strings.index("in the house")] == 0.5 * 4.0 * 2
    strings, weights = by_span[3, 3, 8]                                           # inthe: the pair costs one unit
    assert weights[strings.index("in the")] == 0.5 * 4.0 * 1


class NoChains(OracleLM):
    """the double with a `lexicon_chains` that must not be reached"""

    def lexicon_chains(self, *args, **more):
        raise AssertionError("lexicon_chains called")


def test_defaults_are_what_they_were_and_call_no_chains():
    r, plain = chain_rater(NoChains), chain_rater(OracleLM)
    lex, plain_lex = r.lexicon(ENTRIES), plain.lexicon(ENTRIES)
    contexts = [[170 + i] for i in range(len(TEXTS))]
    called = []
    r.lexicon_chains = lambda *args, **more: called.append(args) or 1 / 0
    for more in (dict(), dict(boundaries=True), dict(boundaries=True, known=True, min_part=1), dict(max_dist=1)):
        settings = dict(dict(max_dist=2, per_word=4, **dict(RULE, **RESCORING)), **more)
        ref = plain.correct_words(TEXTS, plain_lex, contexts, **settings)
        for keywords in (dict(), dict(compounds=0, links=(), max_parts=2), dict(compounds=0, links=("s",))):
            found, rescored, bits = r.correct_words(TEXTS, lex, contexts, **dict(settings, **keywords))
            assert bits.tobytes() == ref[2].tobytes()
            same_rescored(rescored, ref[1])
            for one, other in zip(rescored, ref[1]):
                assert all(getattr(one, name).tobytes() == getattr(other, name).tobytes()
                           for name in ("starts", "ends", "first", "cost0", "cost", "best", "gain"))
    assert not called
    # max_parts without boundaries is not read; with them it is what reaches the chains
    r.correct_words(TEXTS[:1], lex, contexts[:1], max_parts=0, **dict(RULE, **RESCORING))
    assert not called
    with pytest.raises(ZeroDivisionError):
        r.correct_words(TEXTS[:1], lex, contexts[:1], boundaries=True, max_parts=3, **dict(RULE, **RESCORING))
    assert len(called) == 1 and called[0][2:] == (3, 2)


def test_correct_words_value_errors():
    r = chain_rater(OracleLM)
    lex = r.lexicon(ENTRIES)
    contexts = [[170 + i] for i in range(len(TEXTS))]
    for wrong in (dict(compounds=1), dict(compounds=9), dict(compounds=-1), dict(compounds=2, min_part=0), dict(compounds=2, min_part=33),
                  dict(compounds=2, links=["s"] * 9), dict(compounds=2, links=[""]), dict(compounds=2, links=["stst"]),
                  dict(compounds=2, links=["x"]), dict(boundaries=True, max_parts=1), dict(boundaries=True, max_parts=9)):
        with pytest.raises(ValueError):
            r.correct_words(TEXTS, lex, contexts, **wrong)
    with pytest.raises(ValueError):
        r.correct_words(TEXTS, chain_rater(OracleLM).lexicon(ENTRIES), contexts, compounds=2)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_lexicon_compounds_links_and_max_parts(tmp_path, monkeypatch):
    from ocrd_keraslm_amd.scripts import run
    r = chain_rater(OracleLM)
    monkeypatch.setattr(run, "_load", lambda model, incremental=False: r)
    model = tmp_path / "model.h5"
    model.write_bytes(b"")
    files, texts = [], [t for t in TEXTS if t]
    for i, text in enumerate(texts):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        name.write_text(text)
        files.append(str(name))
    contexts = [[170], [174], [178], [182]]
    listing = tmp_path / "words.tsv"
    listing.write_text("".join("%s\t%d\n" % (w, 1000 - i) for i, w in enumerate(ENTRIES)))
    options = ["-s", "4", "-k", "2", "--max-prob", "1", "--min-rank", "0", "--min-suspects", "0", "--max-dist", "2", "--per-word", "4",
               "--left", "12", "--ahead", "3", "--min-gain", "0.5"]
    base = ["lexicon", "-m", str(model), "--lexicon", str(listing), "--apply"]
    ref = chain_rater(OracleLM)
    ref_lex = ref.lexicon(ENTRIES)

    def rows_of(flags, **keywords):
        res = CliRunner().invoke(run.cli, base + flags + options + files)
        assert res.exit_code == 0, res.output + repr(res.exception)
        lines = [json.loads(l) for l in res.output.strip().split("\n")]
        _, found, _ = ref.correct_words(texts, ref_lex, contexts, max_dist=2, per_word=4, **dict(RULE, **RESCORING), **keywords)
        for line, text, one in zip(lines, texts, found):
            assert line["corrected"] == one.apply(text) and len(line["rescored"]) == len(one)
            for row, a, b, new, g in zip(line["rescored"], one.starts, one.ends, one.proposals(), one.gain):
                assert row[:5] == [int(a), int(b), text[int(a):int(b)], new, float(g)]
        return [row for line in lines for row in line["rescored"]]

    both = rows_of(["--boundaries", "--max-parts", "3", "--compounds", "2", "--links", "s,es"], boundaries=True, max_parts=3,
                   compounds=2, links=("s", "es"))      # (as a compound of three, `inthehouse` itself would be left alone)
    splits = rows_of(["--boundaries", "--max-parts", "3"], boundaries=True, max_parts=3)
    alone = rows_of(["--compounds", "3", "--links", "s"], compounds=3, links=("s",))
    plain = rows_of([])
    assert all(len(row) == 6 for row in both + splits) and all(len(row) == 5 for row in alone + plain)
    # a chain candidate is a "split" record; the compounds are gone from the records where they count as entries
    of = lambda rows, word: [row for row in rows if row[2] == word]
    assert of(splits, "inthehouse") and of(splits, "arbeitsamt") and not of(both, "arbeitsamt") and of(both, "inthehouse")
    chosen = [row for row in splits if row[3] is not None and row[3].count(" ") >= 2]
    assert all(row[5] == "split" for row in chosen)
    assert len(of(plain, "bahnhof")) >= len(of(alone, "bahnhof")) == 0
    for wrong in (["--compounds", "1"], ["--compounds", "9"], ["--max-parts", "1"], ["--max-parts", "9"], ["--compounds", "2", "--links", "x"],
                  ["--compounds", "2", "--links", "stst"], ["--compounds", "2", "--links", "s,s,s,s,s,s,s,s,s"]):
        assert CliRunner().invoke(run.cli, base + ["--boundaries"] + wrong + files).exit_code != 0, wrong
