"""Lexicon chains on the GPU (run with -m gpu on an MI355X): kl_lexicon_chains, `HipLM.lexicon_chains`, `Rater.lexicon_chains`
and `Rater.correct_words(compounds=.., links=.., max_parts=..)`.

The kernel is held to its numpy statement (`ratebulk.lexicon_chains_host`, itself held to an enumeration of all chains in
test_lexicon_chains.py) bit for bit: all five outputs are integers.  Every output byte is FILL before a call, and 64 elements
behind each output must keep it.  The shapes are the smallest at which the kernel can go wrong: query lengths at the edges of a
32- and a 64-bit pattern word, pieces at the query's first id, in its middle and at its last, length classes of a lane more
and a lane less than a wave and a round of the workgroup, winners of a piece's minimum scattered over lanes and waves, links
at every place they may and may not stand."""
import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebulk
from tests.test_lexicon import pooled, same_rescored
from tests.test_lexicon_chains import ENTRIES, TEXTS, chain_by_hand, chain_rater, encoded, ids
from tests.test_lexicon_gpu import shuffled, word
from tests.test_lexicon_splits import RESCORING, RULE
from tests.test_rate_bulk_gpu import device, lib_and_stream
from tests.test_rate_window_gpu import make_model, ptr
from tests.test_rate_words_gpu import FILL, KL_ERR_ARG, KL_ERR_WORKSPACE, marked, raw, same_bytes, shifted, up

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
OUTPUTS = ("found", "worst", "entry", "start", "link")


class Chain(object):
    """kl_lexicon_chains on device copies of a lexicon (entries: lists of ids, original index = place in the list) and of
    queries; five outputs of Q, Q * P and Q * P * P entries plus a guard band -- the pattern of test_lexicon_splits_gpu.Cut"""
    NAMES = ("chars", "order", "q_pool", "q_off") + OUTPUTS

    def __init__(self, entries, queries, V, shuffle=None):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        self.V, self.Q = V, len(queries)
        self.layout = shuffled(ratebulk.lexicon_layout_host(*pooled(entries)), shuffle)
        self.queries = pooled(queries)
        some = lambda a: up(a) if len(a) else self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)
        self.src = [some(self.layout[0]), some(self.layout[1]), some(self.queries[0]), up(self.queries[1])]
        self.class_first = np.ascontiguousarray(self.layout[2])
        self.n_ws = self.lib.kl_lexicon_chains_workspace_bytes(self.Q, 8)
        self.ws = self.torch.full((max(self.n_ws, 8),), FILL, dtype=self.torch.uint8, device=self.dev)

    def want(self, links, P, min_part):
        return ratebulk.lexicon_chains_host(*self.queries, *self.layout, self.V, links, P, min_part)

    def run(self, link_ids, P, min_part, room=None, ws_bytes=None, shift=None, table=None, rows=None, **override):
        """link_ids: id lists, or with `rows` the int32 [n, 4] as it stands (what the entry point must refuse)"""
        torch = self.torch
        room = P if room is None else room
        self.out = [marked(self.Q, torch.int32), marked(self.Q * room, torch.int32)] + [marked(self.Q * room * room, torch.int32)
                                                                                       for _ in range(3)]
        self.ws.fill_(FILL)
        cf = self.class_first if table is None else np.ascontiguousarray(table, dtype=np.int64)      # (on the host)
        rows = np.ascontiguousarray(ratebulk.lexicon_links_host(link_ids, self.V) if rows is None else rows, dtype=np.int32).reshape(-1, 4)
        a = dict(zip(self.NAMES, [ptr(t) for t in self.src] + [ptr(t) for t in self.out]), n_chars=len(self.layout[0]), V=self.V,
                 n_q=len(self.queries[0]), Q=self.Q, class_first=ptr(torch.from_numpy(cf)), ws=ptr(self.ws),
                 links=ptr(torch.from_numpy(rows)) if len(rows) else None, n_links=len(rows))
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_lexicon_chains(a["chars"], a["n_chars"], a["order"], a["class_first"], a["V"], a["q_pool"], a["n_q"],
                                          a["q_off"], a["Q"], a["links"], a["n_links"], P, min_part, a["found"], a["worst"],
                                          a["entry"], a["start"], a["link"], a["ws"], self.n_ws if ws_bytes is None else ws_bytes,
                                          self.stream)
        torch.cuda.synchronize()
        return code

    def holds(self, want, Q=None):
        """the outputs are want's for the first Q queries, bit for bit, and everything behind keeps FILL"""
        Q = self.Q if Q is None else Q
        return all(same_bytes(t, np.ascontiguousarray(w).reshape(-1), Q * (w.size // max(len(w), 1)))
                   for t, w in zip(self.out, want))

    def is_statement(self, links, P, min_part):
        want = self.want(links, P, min_part)
        assert self.run(links, P, min_part) == 0
        for t, w, name in zip(self.out, want, OUTPUTS):
            assert same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size), (name, links, P, min_part)
        return want

    def untouched(self):
        return all((raw(t) == FILL).all() for t in self.out) and (raw(self.ws) == FILL).all()


def bit(p):
    return 1 << (p - 1)


LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64)


def lengths_case():
    """queries of 1, 2, 3, 31, 32, 33, 63 and 64 ids (and of 0 and 65); per query the pieces q[:s], q[s:t] and q[t:] -- at its
    first id, in the middle and ending at its last --, the whole query, its first id alone, and its halves where m is even;
    entries of 64 ids beside them"""
    rng = np.random.default_rng(50)
    V = 8
    queries, entries, cuts = [], [], {}
    for m in LENGTHS:
        q = word(rng, V, m)
        queries.append(q)
        s, t = max(1, m // 3), max(2, 2 * m // 3)
        cuts[m] = (s, t)
        entries += [word(rng, V, 64), list(q), q[:s], q[s:t], q[t:], q[:1], q[:m // 2], q[m // 2:]]      # (no ids: left out)
        entries += [word(rng, V, max(1, min(64, m // 2 + int(rng.integers(-3, 4))))) for _ in range(4)]
    queries += [[], word(rng, V, 65)]
    return V, entries, queries, cuts


@pytest.mark.parametrize("narrow", ["1", "0"])
def test_query_lengths_at_the_edges_of_the_pattern_word_and_pieces_at_both_ends(narrow, monkeypatch):
    """(narrow 1, the default: queries of at most 32 ids run on a 32-bit pattern word; KL_LEXICON_NARROW=0: all on 64 bits)"""
    monkeypatch.setenv("KL_LEXICON_NARROW", narrow)
    V, entries, queries, cuts = lengths_case()
    chain = Chain(entries, queries, V)
    found, worst, entry, start, link = chain.is_statement([], 4, 1)
    for row, m in enumerate(LENGTHS):
        s, t = cuts[m]
        assert found[row] & bit(1) and entries[entry[row, 0, 0]] == queries[row]
        if m >= 3:
            assert found[row] & bit(3) and found[row] & bit(2), m
        if m >= 2 and m % 2 == 0:
            assert found[row] & bit(2), m
    assert found[-2:].tolist() == [0, 0] and all((a[-2:] == -1).all() for a in (worst, entry, start, link))
    chain.is_statement([], 8, 2)
    chain.is_statement([[3], [5, 1]], 2, 1)
    # min_part 32: the halves of the query of 64 ids alone; above m: no row, and nothing read
    found, worst, entry, start, link = chain.is_statement([], 2, 32)
    assert found.tolist() == [0, 0, 0, 0, bit(1), bit(1), bit(1), bit(1) | bit(2), 0, 0] and start[7, 1].tolist() == [0, 32]
    found = chain.is_statement([], 3, 4)[0]
    assert found[:3].tolist() == [0, 0, 0] and (found[3:8] & bit(1)).all()


def classes_case():
    """length classes of 63, 64, 65, 255, 256 and 257 entries (and one of 700), shuffled within; the queries are two and three
    entries run together, so that the winner of a piece comes from any lane and wave, and every entry has twins at scattered
    indices, so that the least index must win"""
    rng = np.random.default_rng(52)
    V = 3
    sizes = {2: 63, 3: 64, 4: 65, 5: 255, 6: 256, 7: 257, 8: 700}
    entries = [word(rng, V, L) for L, n in sizes.items() for _ in range(n)]
    entries = [entries[i] for i in rng.permutation(len(entries))]
    pick = lambda L, which: entries[int(np.nonzero([len(e) == L for e in entries])[0][which])]
    queries = [pick(L, -1) + pick(M, -1) for L in sizes for M in (2, 5, 8)]      # the last lanes of the classes
    queries += [pick(L, int(rng.integers(0, n))) + pick(9 - L if L < 8 else 8, 0) + pick(L, 0) for L, n in sizes.items()]
    queries += [word(rng, V, int(rng.integers(4, 25))) for _ in range(12)]
    return V, sizes, entries, queries


def test_class_sizes_across_a_wave_and_a_round_of_the_workgroup():
    V, sizes, entries, queries = classes_case()
    chain = Chain(entries, queries, V, shuffle=np.random.default_rng(53))
    assert np.diff(chain.layout[2])[2:9].tolist() == list(sizes.values())
    found, worst, entry, start, link = chain.is_statement([], 4, 2)
    assert (found[:len(queries) - 12] != 0).all() and (found & bit(3)).any() and (found & bit(4)).any()
    # twins: the index named is the least of the identical entries
    first = {}
    for i, e in enumerate(entries):
        first.setdefault(tuple(e), i)
    named = [(int(i), entries[int(i)]) for i in entry.reshape(-1) if i >= 0]
    assert all(first[tuple(e)] == i for i, e in named) and len(set(i for i, _ in named)) > 40
    position = dict((int(e), p) for p, e in enumerate(chain.layout[1]))
    lanes = [position[i] - int(chain.layout[2][len(e)]) for i, e in named]
    assert len(set(p % 64 for p in lanes)) > 32 and len(set(p // 64 % 4 for p in lanes)) == 4      # lanes, and all four waves
    chain.is_statement([[0], [1, 2]], 8, 2)
    chain.is_statement([], 3, 5)


def test_every_row_of_abab_and_the_tie_rule():
    """`abab..` over the entries ab, abab, ..: a chain of p parts exists for every p up to the number of units, its bottleneck
    is ceil(units / p) - 1, and among the chains of least bottleneck the one with the longest last piece is kept"""
    V = 4
    entries = [[0, 1] * n for n in range(1, 33)] + [[2, 3]]
    queries = [[0, 1] * 4, [0, 1] * 32, [0, 1] * 4 + [2], [2, 3, 2, 3], [0, 1, 2, 3], [0, 1] * 5]
    chain = Chain(entries, queries, V)
    for P in (2, 8):
        found, worst, entry, start, link = chain.is_statement([], P, 1)
        assert found.tolist() == [0b1111 & (bit(P + 1) - 1), bit(P + 1) - 1, 0, bit(2), bit(2), 0b11111 & (bit(P + 1) - 1)]
        assert (link == -1).all()
        for p in range(1, P + 1):
            w = -(-32 // p) - 1
            assert worst[1, p - 1] == w and entry[1, p - 1, p - 1] == w and start[1, p - 1, p - 1] == 64 - 2 * (w + 1)
        assert entry[0, :2].tolist() == [[3] + [-1] * (P - 1), [1, 1] + [-1] * (P - 2)] and start[0, 1, :2].tolist() == [0, 4]
        assert entry[4, 1, :2].tolist() == [0, 32] and entry[3, 1, :2].tolist() == [32, 32]
    assert entry[0, 2, :4].tolist() == [0, 0, 1, -1] and start[0, 2, :4].tolist() == [0, 2, 4, -1]
    assert entry[0, 3, :4].tolist() == [0, 0, 0, 0] and start[0, 3, :4].tolist() == [0, 2, 4, 6]
    assert entry[5, 1, :2].tolist() == [1, 2] and entry[5, 2, :3].tolist() == [0, 1, 1]      # (2 + 3 units; 1 + 2 + 2)
    chain.is_statement([], 8, 2)
    chain.is_statement([], 8, 3)      # (no piece of one unit)


def test_eight_parts_and_nine():
    rng = np.random.default_rng(54)
    V = 8
    eight, nine = word(rng, V, 64), word(rng, V, 63)
    entries = [eight[8 * k:8 * k + 8] for k in range(8)] + [nine[7 * k:7 * k + 7] for k in range(9)]
    entries = [entries[i] for i in rng.permutation(len(entries))]
    chain = Chain(entries, [eight, nine, eight[:56], nine[7:]], V)
    found, worst, entry, start, link = chain.is_statement([], 8, 1)
    assert found.tolist() == [bit(8), 0, bit(7), bit(8)] and start[0, 7].tolist() == list(range(0, 64, 8))
    assert [entries[e] for e in entry[0, 7]] == [eight[8 * k:8 * k + 8] for k in range(8)] and worst[0, 7] == entry[0, 7].max()
    assert (worst[1] == -1).all() and (entry[1] == -1).all() and (start[1] == -1).all() and (link[1] == -1).all()
    assert chain.is_statement([], 7, 7)[0].tolist() == [0, 0, bit(7), 0]


def test_links_where_they_may_and_may_not_stand():
    V = 26
    entries = [ids(e) for e in ("a", "cd", "ab", "c", "arbeit", "amt")]
    queries = [ids(q) for q in ("axcd", "abxyzc", "abx", "xab", "xcd", "abxc", "abxyc", "axyzcd", "abqqqcxcd", "aqa", "abxxc", "abc",
                                "arbeitsamt", "axcdxyab")]
    links = [ids(l) for l in ("x", "x", "xy", "xyz", "q", "qq", "qqq", "s")]
    chain = Chain(entries, queries, V)
    found, worst, entry, start, link = chain.is_statement(links, 3, 1)
    two = lambda row: (entry[row, 1, :2].tolist(), start[row, 1, :2].tolist(), int(link[row, 1, 0]))
    assert two(0) == ([0, 1], [0, 2], 0)                  # right behind a one-id first piece; of two identical links the first
    assert two(1) == ([2, 3], [0, 5], 3)                  # three ids, right in front of the last piece
    assert found[2:5].tolist() == [0, 0, 0]               # at the word's end; with nothing in front of it (twice)
    assert two(5) == ([2, 3], [0, 3], 0) and two(6) == ([2, 3], [0, 4], 2) and two(7) == ([0, 1], [0, 4], 3)
    assert found[8] == bit(3) and link[8, 2, :2].tolist() == [6, 0] and start[8, 2].tolist() == [0, 5, 7]
    assert two(9) == ([0, 0], [0, 2], 4) and found[10] == 0 and two(11) == ([2, 3], [0, 2], -1)      # (no two links in a row)
    assert two(12) == ([4, 5], [0, 7], 7)
    assert found[13] == bit(3) and link[13, 2, :2].tolist() == [0, 2] and entry[13, 2].tolist() == [0, 1, 2]
    # without links only the direct chain is left
    assert chain.is_statement([], 3, 1)[0].tolist() == [0] * 11 + [bit(2), 0, 0]
    assert chain.is_statement(links[2:5], 2, 2)[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert chain.is_statement(links[:1], 2, 1)[0].tolist() == [2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 2, 0, 0]
    # `arbeits` an entry too: the bottleneck decides, on equal keys the chain without a link -- visited first -- is kept
    for lexicon, want_entry, want_link in ((["arbeits", "arbeit", "amt"], [0, 2], -1), (["arbeit", "amt", "arbeits"], [0, 1], 0),
                                           (["amt", "arbeit", "arbeits"], [1, 0], 0), (["arbeit", "arbeits", "amt"], [1, 2], -1)):
        found, worst, entry, start, link = Chain([ids(e) for e in lexicon], [ids("arbeitsamt")], V).is_statement([ids("s")], 2, 2)
        assert found.tolist() == [bit(2)] and entry[0, 1].tolist() == want_entry and link[0, 1, 0] == want_link, lexicon


def test_ids_outside_the_table_two_calls_and_fewer_queries():
    """V, -1 and 2^31 - 1 equal nothing, themselves included, and never index the table; a second call gives the same bytes;
    nothing behind Q is written"""
    rng = np.random.default_rng(55)
    for V in (8, 4096):
        odd = [V, -1, INT_MAX, 0, V - 1]
        entries = [[h, 1, 2] for h in odd] + [[2, 1, h] for h in odd] + [[h] for h in odd] + [word(rng, V, int(rng.integers(1, 7))) for _ in range(300)]
        queries = [[i for e in rng.integers(0, len(entries), int(rng.integers(1, 5))) for i in entries[int(e)]] for _ in range(60)]
        queries += [[V, 1, 2, 2, 1, V], [0, 1, 2, V - 1, 1, 2], [-2 ** 31, 3], [INT_MAX] * 64, [V - 1, 0, 0]]
        chain = Chain(entries, queries, V, shuffle=rng)
        links = [[0], [V - 1, 1]]
        want = chain.is_statement(links, 4, 1)
        first = [raw(t).copy() for t in chain.out]
        assert (want[0] > 0).sum() > 30 and want[0][-5:].tolist()[:1] == [0] and want[0][-4] & 2 and want[0][-2] == 0 and want[0][-1] != 0
        assert chain.run(links, 4, 1) == 0 and all(np.array_equal(x, raw(t)) for x, t in zip(first, chain.out))
        assert chain.run(links, 4, 1, Q=7) == 0 and chain.holds(want, Q=7)
        Chain(entries, queries[:1], V).is_statement(links, 4, 1)


def test_errors_return_before_any_launch():
    rng = np.random.default_rng(56)
    V = 8
    entries = [word(rng, V, int(rng.integers(1, 9))) for _ in range(200)]
    queries = [entries[i] + entries[i + 1] + entries[i + 2] for i in range(20)]
    chain = Chain(entries, queries, V)
    cf = chain.class_first
    assert chain.n_ws % 8 == 0 and chain.n_ws == chain.lib.kl_lexicon_chains_workspace_bytes(1, 2)
    down, short, late, none = cf.copy(), cf.copy(), cf.copy(), cf * 0
    down[5] = down[4] - 1 if down[4] > 0 else down[6] + 1          # decreases
    short[65] += 1                                                   # one entry more than n_chars holds ids for
    late[1] = 1                                                      # class_first[1] != 0
    links = [[1], [2, 3]]
    cases = [dict(table=down), dict(table=short), dict(table=late), dict(table=none),
             dict(n_chars=len(chain.layout[0]) + 1), dict(V=0), dict(V=4097), dict(Q=0), dict(Q=2 ** 31),
             dict(n_q=2 ** 40 + 1), dict(n_chars=2 ** 40 + 1)]
    cases += [{name: None} for name in chain.NAMES + ("class_first", "ws", "links")]
    cases += [dict(shift={name: 2}) for name in ("chars", "order", "q_pool") + OUTPUTS]
    cases += [dict(shift={name: 4}) for name in ("q_off", "class_first", "ws")]
    cases += [dict(n_links=-1), dict(n_links=9)]
    cases += [dict(rows=[[0, 1, 0, 0]]), dict(rows=[[4, 1, 1, 1]]), dict(rows=[[-1, 1, 1, 1]]), dict(rows=[[1, 1, 0, 0], [2, 1, V, 0]]),
              dict(rows=[[3, 1, 2, -1]]), dict(rows=[[1, INT_MAX, 0, 0]])]
    for case in cases:
        assert chain.run(links, 3, 2, **case) == KL_ERR_ARG, case
        assert chain.untouched(), case
    for P, min_part in ((1, 2), (0, 2), (-1, 2), (9, 2), (3, 0), (3, -1), (3, 33)):
        assert chain.run(links, P, min_part, room=8) == KL_ERR_ARG and chain.untouched(), (P, min_part)
    assert chain.run(links, 3, 2, ws_bytes=chain.n_ws - 1) == KL_ERR_WORKSPACE and chain.untouched()
    # an unused id of a link is not looked at
    assert chain.run(links, 3, 2, rows=[[1, 1, -5, V], [2, 2, 3, INT_MAX]]) == 0 and chain.holds(chain.want(links, 3, 2))
    assert chain.is_statement(links, 3, 2)[0].max() >= 1
    chain.is_statement([[1]] * 8, 8, 1)


# ---------------------------------------------------------------------------------------------- engine and Rater
def test_engine_wrapper_and_rater_lexicon_chains():
    from ocrd_keraslm_amd.lib import hipabi
    from tests.test_rater_golden import hip_factory
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 1)
    rng = np.random.default_rng(57)
    V = 20
    entries = [word(rng, V, int(rng.integers(1, 7))) for _ in range(500)]
    queries = [[i for e in rng.integers(0, 500, int(rng.integers(1, 5))) for i in entries[int(e)]] for _ in range(50)] + [[], [3] * 65]
    chars, order, class_first = ratebulk.lexicon_layout_host(*pooled(entries))
    q_pool, q_off = pooled(queries)
    links = [[4], [5, 6]]
    want = ratebulk.lexicon_chains_host(q_pool, q_off, chars, order, class_first, V, links, 5, 2)
    got = lm.lexicon_chains(up(chars), up(order), class_first, V, up(q_pool), up(q_off), links, 5, 2)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got)
    assert [tuple(t.shape) for t in got] == [(52,), (52, 5)] + [(52, 5, 5)] * 3
    for g, r in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), r)
    again = lm.lexicon_chains(up(chars), up(order), class_first, V, up(q_pool), up(q_off), ratebulk.lexicon_links_host(links, V), 5, 2)
    assert all(np.array_equal(a.cpu().numpy(), r) for a, r in zip(again, want)) and want[0].max() > 1
    for wrong in (dict(chars=up(chars).long()), dict(q_off=up(q_off).int()), dict(order=up(order)[::2]), dict(q_pool=torch.from_numpy(q_pool)),
                  dict(class_first=class_first[:-1]), dict(P=1), dict(P=9), dict(min_part=0), dict(min_part=33), dict(V=4097),
                  dict(links=[[V]]), dict(links=[[]]), dict(links=[[1, 2, 3, 4]]), dict(links=[[1]] * 9)):
        a = dict(dict(chars=up(chars), order=up(order), class_first=class_first, V=V, q_pool=up(q_pool), q_off=up(q_off), links=links,
                      P=5, min_part=2), **wrong)
        with pytest.raises(hipabi.KlError):
            lm.lexicon_chains(a["chars"], a["order"], a["class_first"], a["V"], a["q_pool"], a["q_off"], a["links"], a["P"], a["min_part"])
    # the Rater: normalised, unique, spread back over the duplicates; the device copy of the lexicon is made once
    hip = chain_rater(hip_factory)
    assert hasattr(hip.model, "lexicon_chains")
    lex = hip.lexicon(ENTRIES)
    words = ["arbeitsamt", "inthehouse", "bahnhof", "house", "", "arbeitsamt", "reisebahnhof", "in?house", "ab" * 40, "hause", "inahouse"]
    chains = hip.lexicon_chains(words, lex, max_parts=3, min_part=2, links=("s",))
    held = lex.on_device(hip.model)
    want = ratebulk.lexicon_chains_host(*encoded(hip, words), lex.chars, lex.order, lex.class_first, hip.voc_size,
                                        [[hip.mapping[0]["s"]]], 3, 2)
    for g, r in zip((chains.found, chains.worst, chains.entry, chains.start, chains.link), want):
        assert g.dtype == np.int32 and np.array_equal(g, r)
    assert chains.strings(0) == ["arbeits amt"] == chains.strings(5) and chains.strings(1) == ["in the house"] and chains.parts(3) == 1
    again = hip.lexicon_chains(words[:3], lex, max_parts=2, min_part=1)
    assert all(a is b for a, b in zip(held, lex.on_device(hip.model))) and again.strings(2) == ["bahn hof"] and again.found[0] == 0
    none = hip.lexicon_chains([], lex)
    assert len(none) == 0 and none.entry.shape == (0, 4, 4)


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_rater_correct_words_with_compounds_is_the_chain_with_the_host_statements(precision):
    """texts with planted compounds and words that lost two spaces: the same edits, candidates, choices and costs as the chain
    written out by hand in test_lexicon_chains.py, whose look-ups are the numpy statements -- rating and rescoring are the
    same device code on both sides, so the costs are identical, as in test_lexicon_splits_gpu's composed call"""
    from tests.test_rater_golden import hip_factory
    hip = chain_rater(hip_factory)
    assert hasattr(hip.model, "lexicon_chains") and hasattr(hip.model, "lexicon_splits")
    lex = hip.lexicon(ENTRIES)
    contexts = [[170 + i] for i in range(len(TEXTS))]
    for known, compounds in ((False, 3), (True, 3), (False, 2)):
        found, rescored, bits = hip.correct_words(TEXTS, lex, contexts, max_dist=2, per_word=4, known=known, boundaries=True, min_part=2,
                                                  compounds=compounds, links=("s",), max_parts=3, precision=precision,
                                                  **dict(RULE, **RESCORING))
        ref_found, edits, ref_rescored, ref_bits = chain_by_hand(hip, TEXTS, contexts, lex, 2, 4, known, 2, compounds, ("s",), 3,
                                                                 dict(RULE, precision=precision), dict(RESCORING, precision=precision))
        assert np.array_equal(bits, ref_bits)
        for one, ref in zip(found, ref_found):
            assert one.spans() == ref.spans() and np.array_equal(one.bits, ref.bits)
        same_rescored(rescored, ref_rescored)
        by_span = dict(((i, a, b), c) for i, a, b, c in edits)
        assert ((0, 2, 12) in by_span) == known and ("in the house" in by_span.get((0, 13, 23), [])) == (known or compounds == 2)
        assert ("out the amt" in by_span.get((1, 11, 20), [])) == (known or compounds == 2)
        assert sum(len(one) for one in rescored) == len(edits) > 0 and sum(int((one.best >= 0).sum()) for one in rescored) > 0
    assert hip.model.states.shape[0] == 1 and not hip.model.states.cpu().numpy().any()
