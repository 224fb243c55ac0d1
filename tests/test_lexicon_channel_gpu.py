"""The weighted lexicon look-up on the GPU (run with -m gpu on an MI355X): kl_lexicon_channel, `HipLM.lexicon_channel`,
`Rater.lexicon_neighbours(channel=..)`, `Rater.rescore(prior=..)`, `Rater.correct_words(channel=..)` and
`keraslm-rate lexicon --channel`.

The kernel is held to its numpy statement (`ratebulk.lexicon_channel_host`, itself held to a shortest path in
test_lexicon_channel.py) bit for bit: all four outputs are integers.  Every output byte is FILL before a call, and 64 elements
behind each output must keep it.  The shapes are the smallest at which the kernel can go wrong: query lengths at the edges of a
rule's reach, of the steps in which the lanes that walk go down (256 up to 15 ids, 192 up to 21, 128 up to 32, 64 beyond) and of
the ring; rules that match at the first and at the last ids; more (rule, row) pairs than the active list holds; costs that
pass 16 bits; length classes that only the rules' prices open."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.test_lexicon import lexicon_words, mutate, pooled, same_rescored
from tests.test_lexicon_channel import channel_case, composed_channel, prior_is_added, records, winner_changes
from tests.test_lexicon_gpu import INT_MAX, Look, shuffled, word
from tests.test_rate_bulk_gpu import device, lib_and_stream, random_text, small_rater
from tests.test_rate_suspects import contract_texts
from tests.test_rate_window_gpu import make_model, ptr
from tests.test_rate_words_gpu import FILL, KL_ERR_ARG, KL_ERR_WORKSPACE, marked, raw, same_bytes, shifted, up

pytestmark = pytest.mark.gpu


class Chan(object):
    """kl_lexicon_channel on device copies of a lexicon (entries: lists of ids, original index = place in the list), of
    queries and of rules ([(src ids, tgt ids, cost)], or the raw arrays); four outputs of Q (Q * K) entries plus a guard band"""
    NAMES = ("chars", "order", "q_pool", "q_off", "rules", "rule_cost", "exact", "found", "cand", "cost")

    def __init__(self, entries, queries, V, rules=(), shuffle=None):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        self.V, self.Q = V, len(queries)
        self.layout = shuffled(ratebulk.lexicon_layout_host(*pooled(entries)), shuffle)
        self.queries = pooled(queries)
        self.some = lambda a: up(a) if len(a) else self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)
        self.src = [self.some(self.layout[0]), self.some(self.layout[1]), self.some(self.queries[0]), up(self.queries[1])]
        self.class_first = np.ascontiguousarray(self.layout[2])
        self.set_rules(rules)

    def set_rules(self, rules):
        self.rules = records(rules) if isinstance(rules, (list, tuple)) and (not rules or len(rules[0]) == 3) else rules
        self.R = len(self.rules[1])
        self.rules_d = [self.some(self.rules[0].reshape(-1)), self.some(self.rules[1])]
        self.n_ws = self.lib.kl_lexicon_channel_workspace_bytes(self.Q, 16, self.R)
        self.ws = self.torch.full((max(self.n_ws, 8),), FILL, dtype=self.torch.uint8, device=self.dev)

    def want(self, unit, max_cost, K):
        return ratebulk.lexicon_channel_host(*self.queries, *self.layout, self.V, self.rules[0], self.rules[1], unit, max_cost, K)

    def run(self, unit, max_cost, K, room=None, ws_bytes=None, shift=None, table=None, **override):
        torch = self.torch
        room = K if room is None else room
        self.out = [marked(self.Q, torch.int32), marked(self.Q, torch.int32), marked(self.Q * room, torch.int32),
                    marked(self.Q * room, torch.int32)]
        self.ws.fill_(FILL)
        cf = self.class_first if table is None else np.ascontiguousarray(table, dtype=np.int64)      # (on the host)
        a = dict(zip(self.NAMES, [ptr(t) for t in self.src + self.rules_d + self.out]), n_chars=len(self.layout[0]), V=self.V,
                 n_q=len(self.queries[0]), Q=self.Q, R=self.R, class_first=ptr(torch.from_numpy(cf)), ws=ptr(self.ws))
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_lexicon_channel(a["chars"], a["n_chars"], a["order"], a["class_first"], a["V"], a["q_pool"], a["n_q"],
                                           a["q_off"], a["Q"], a["rules"], a["rule_cost"], a["R"], unit, max_cost, K, a["exact"],
                                           a["found"], a["cand"], a["cost"], a["ws"], self.n_ws if ws_bytes is None else ws_bytes,
                                           self.stream)
        torch.cuda.synchronize()
        return code

    def holds(self, want, Q=None):
        """the outputs are want's for the first Q queries, bit for bit, and everything behind keeps FILL"""
        Q = self.Q if Q is None else Q
        return all(same_bytes(t, np.ascontiguousarray(w).reshape(-1), Q * (w.size // max(len(w), 1)))
                   for t, w in zip(self.out, want))

    def is_statement(self, unit, max_cost, K, want=None):
        want = self.want(unit, max_cost, K) if want is None else want
        assert self.run(unit, max_cost, K) == 0
        for t, w, name in zip(self.out, want, ("exact", "found", "cand", "cost")):
            assert same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size), (name, unit, max_cost, K)
        return want

    def untouched(self):
        return all((raw(t) == FILL).all() for t in self.out) and (raw(self.ws) == FILL).all()


def reached(want, row, entry):
    """the cost at which the statement lists `entry` for query `row`, None if it does not"""
    near = dict(zip(want[2][row].tolist(), want[3][row].tolist()))
    return near.get(entry)


LENGTHS = (1, 2, 4, 5, 15, 16, 21, 22, 31, 32, 33, 63, 64)


def test_query_lengths_and_rules_at_the_first_and_the_last_ids():
    """queries of 1, 2, 4, 5, 15, 16, 31, 32, 63 and 64 ids (21 | 22 and 32 | 33: where the lanes that walk go down; 0 and 65:
    nothing); per query entries reached by a rule that matches at the first ids of both words (i == s, j == t: nothing in
    front of either may be read), by one at the last ids, by two back to back and by a deletion rule at either end; ids 6 and
    7 stand in targets only"""
    rng = np.random.default_rng(50)
    V, unit = 8, 100
    queries, entries, rules, marks = [], [], [], {}
    for m in LENGTHS:
        q = word(rng, 6, m)
        s = min(m, 4)
        head, tail = ([6, 7, 7, 6], q[:s], 11), (q[-s:], [7, 6, 6], 13)
        marks[m] = len(entries)
        entries.append(list(q))                                             # 0: itself
        entries.append(head[0] + q[s:])                                     # 1: the first s ids read four others
        entries.append(q[:-s] + tail[1])                                    # 2: the last s ids read three others
        rules += [(head[1], head[0], head[2]), tail]
        if m >= 2:
            a = max(1, min(m // 2, 3))
            first, second = (q[:a], [7, 7], 17), (q[a:a + min(m - a, 2)], [6], 19)
            rules += [first, second]
            entries.append(first[1] + second[1] + q[a + len(second[0]):])   # 3: two rules back to back, from the first id
            rules += [(q[:1], [], 23), (q[-1:], [], 29)]
            entries.append(q[1:])                                           # 4, 5: a deletion rule at either end
            entries.append(q[:-1])
        entries += [word(rng, 6, max(1, min(64, m + int(rng.integers(-3, 4))))) for _ in range(5)]
        queries.append(q)
    queries += [[], word(rng, V, 65)]
    chan = Chan(entries, queries, V, rules)
    assert chan.R == len(rules) > 60
    exact, found, cand, cost = want = chan.is_statement(unit, 99, 16)
    for row, m in enumerate(LENGTHS):
        at = marks[m]
        assert exact[row] == at
        assert reached(want, row, at + 1) == 11 and (m <= 4 or reached(want, row, at + 2) == 13), m
        if m >= 2:
            assert reached(want, row, at + 3) <= 36 and reached(want, row, at + 4) <= 23 and reached(want, row, at + 5) <= 29, m
    assert exact[-2:].tolist() == [-1, -1] and found[-2:].tolist() == [0, 0] and (cand[-2:] == -1).all() and (cost[-2:] == -1).all()
    chan.is_statement(unit, 250, 16)      # (plain edits beside the rules)
    chan.is_statement(unit, 0, 3)


def test_a_cheaper_rule_a_dearer_rule_and_a_rule_that_costs_nothing():
    V, unit = 8, 16
    q = [1, 2, 3, 1, 2, 3]
    rules = [([2], [4], 10),            # cheaper than the substitution
             ([3], [5], 40),            # dearer: the plain substitution wins
             ([1], [6], 0),             # costs nothing
             ([1, 2], [7], 3)]
    entries = [[1, 4, 3, 1, 2, 3], [1, 2, 5, 1, 2, 3], [6, 2, 3, 1, 2, 3], [6, 2, 3, 6, 2, 3], list(q), [7, 3, 7, 3], [6, 4, 5, 7, 3],
               [0] * 6]
    chan = Chan(entries, [q], V, rules)
    exact, found, cand, cost = chan.is_statement(unit, 64, 8)
    assert exact[0] == 4 and found[0] == 6
    # the entries at cost 0 are not identical: they are candidates, come first, and `exact` is not theirs
    assert cand[0, :6].tolist() == [2, 3, 5, 0, 1, 6] and cost[0, :6].tolist() == [0, 0, 6, 10, 16, 29]
    alone = Chan(entries[:4], [q], V, rules)
    assert alone.is_statement(unit, 64, 8)[0][0] == -1


def test_classes_that_only_the_rules_open():
    """rules that lengthen by 3 and shorten by 4, max_cost below one unit: the entries of m + 3, m + 6, m - 4 and m - 8 ids are
    found; a rule that costs nothing opens every class of its side; with unit 1 and no rules the window is max_cost"""
    V = 6
    q = [1, 2, 3, 4] * 3
    rules = [([1], [5, 5, 5, 1], 30), ([1, 2, 3, 4], [], 40)]
    entries = [[5, 5, 5, 1, 2, 3, 4] + q[4:], [5, 5, 5, 1, 2, 3, 4] * 2 + q[8:], q[4:], q[8:], q + [0], q[:-1], [5] * 12]
    chan = Chan(entries, [q], V, rules)
    exact, found, cand, cost = chan.is_statement(100, 99, 8)
    assert found[0] == 4 and cand[0, :4].tolist() == [0, 2, 1, 3] and cost[0, :4].tolist() == [30, 40, 60, 80]
    assert [len(entries[e]) - len(q) for e in cand[0, :4]] == [3, -4, 6, -8]
    free = rules + [([4], [], 0), ([2], [2, 0, 0, 0], 0)]
    far = Chan(entries + [[1, 2, 3], [2, 0, 0, 0] * 3], [q, [2, 2, 2]], V, free)
    want = far.is_statement(100, 99, 8)
    assert reached(want, 0, 7) == 80 and reached(want, 0, 5) == 0 and reached(want, 1, 8) == 0
    plain = Chan([q[:k] for k in range(1, 13)] + [q + [5] * k for k in range(1, 10)], [q], V)
    for max_cost in (0, 3, 8):
        assert plain.is_statement(1, max_cost, 16)[1][0] == min(max_cost, 11) + min(max_cost, 9)


def test_more_pairs_than_the_active_list_holds_and_the_rules_in_any_order():
    """one source with 1024 targets on a query of 64 equal ids -- every rule active in every row: 65 536 (rule, row) pairs --,
    then 1024 distinct sources of which a query holds a few; then the same rules shuffled: the same bytes"""
    rng = np.random.default_rng(51)
    V = 4096
    q = [9] * 64
    targets = [[1000 + n, 2000 + (n % 7)][:1 + n % 2] + [3000 + n] * (n % 3) for n in range(1024)]
    targets[7] = []                                                         # (the source dropped: 12)
    rules = [([9], t, 5 + n % 50) for n, t in enumerate(targets)]
    assert len(set(tuple(t) for t in targets)) == 1024 and max(len(t) for t in targets) == 4
    entries = [targets[0] + q[1:], q[:63] + targets[1020], q[:31] + targets[500] + q[34:], q[:20] + targets[333] + q[22:],
               q[:10] + targets[6] + targets[12] + q[12:], list(q), q[:-1], [8] * 64]      # (two classes: every cell loops over all rules)
    assert [len(e) for e in entries[:5]] == [64] * 5
    chan = Chan(entries, [q], V, rules)
    assert chan.R == 1024
    want = chan.is_statement(200, 150, 16)
    assert want[0].tolist() == [5] and want[1].tolist() == [6]
    assert [reached(want, 0, e) for e in (0, 1, 2, 3, 4, 6)] == [5, 25, 29, 50, 28, 12]
    first = [raw(t).copy() for t in chan.out]
    perm = rng.permutation(1024)
    chan.set_rules((chan.rules[0][perm], chan.rules[1][perm]))
    assert chan.run(200, 150, 16) == 0 and all(np.array_equal(x, raw(t)) for x, t in zip(first, chan.out))
    # 1024 distinct sources: the list holds the few that stand in a query
    sources = [[n // 32 + 10, n % 32 + 10] for n in range(1024)]
    rules = [(s, [50 + n % 5] * (n % 5), 3 + n % 40) for n, s in enumerate(sources)]
    queries = [word(rng, 32, m) for m in (3, 9, 17, 40, 64)]
    queries = [[c + 10 for c in w] for w in queries]
    entries = []
    for w in queries:
        for p in range(0, len(w) - 1, 5):
            n = (w[p] - 10) * 32 + w[p + 1] - 10
            entries.append(w[:p] + rules[n][1] + w[p + 2:])
        entries.append(list(w))
    entries = [e for e in entries if e]
    chan = Chan(entries, queries, V, rules, shuffle=rng)
    want = chan.is_statement(60, 59, 16)
    assert (want[0] >= 0).all() and want[1].min() >= 1 and want[3].max() < 60
    first = [raw(t).copy() for t in chan.out]
    perm = rng.permutation(1024)
    chan.set_rules((chan.rules[0][perm], chan.rules[1][perm]))
    assert chan.run(60, 59, 16) == 0 and all(np.array_equal(x, raw(t)) for x, t in zip(first, chan.out))


def test_costs_beyond_sixteen_bits_saturate():
    """unit = max_cost = 4095 on words of 64 ids with nothing in common: the plain cost is 64 * 4095; beside them one entry at
    exactly 4095, and with a rule one at 4095 through it"""
    V = 8
    q = [1] * 64
    chan = Chan([[2] * 64, [3] * 63, [4] * 60], [q], V)
    exact, found, cand, cost = chan.is_statement(4095, 4095, 4)
    assert exact[0] == -1 and found[0] == 0 and (cand == -1).all() and (cost == -1).all()
    chan = Chan([[2] * 64, q[:30] + [5] + q[31:], [3] * 63, q[:-1], q[:20] + [6, 6] + q[22:], q[:20] + [6, 6] + q[22:-1]], [q], V,
                [([1, 1], [6, 6], 4095), ([1], [7], 4095)])
    exact, found, cand, cost = chan.is_statement(4095, 4095, 4)
    assert found[0] == 3 and cand[0].tolist() == [1, 3, 4, -1] and cost[0].tolist() == [4095, 4095, 4095, -1]


def test_class_sizes_across_a_wave_and_a_round_of_the_lanes_that_walk():
    """256 lanes walk for a query of up to 15 ids, 192 up to 21, 128 up to 32, 64 beyond: classes of a lane fewer than, equal to
    and a lane more than a wave and such a round"""
    rng = np.random.default_rng(52)
    V = 3
    for m, sizes in ((6, {3: 1, 4: 63, 5: 64, 6: 65, 7: 255, 8: 256, 9: 257, 10: 600}), (20, {19: 191, 20: 192, 21: 193}),
                     (30, {29: 127, 30: 128, 31: 129, 32: 300}), (64, {62: 129, 63: 63, 64: 65})):
        root = word(rng, V, 64)
        entries = [mutate(rng, root[:L], V, 2)[:L] for L, n in sizes.items() for _ in range(n)]
        entries = [e + root[len(e):L] for e, L in zip(entries, [L for L, n in sizes.items() for _ in range(n)])]
        entries = [[min(max(c, 0), V - 1) for c in e] for e in entries]
        entries = [entries[i] for i in rng.permutation(len(entries))]
        lengths = sorted(sizes)
        queries = [root[:m], mutate(rng, root[:m], V, 1)]
        queries += [entries[int(np.nonzero([len(e) == L for e in entries])[0][-1])] for L in lengths]      # the last lane of every class
        chan = Chan(entries, queries, V, [([0], [1, 1], 1), ([2, 2], [0], 2), ([1], [], 4)])
        assert np.diff(chan.layout[2])[lengths[0]:lengths[-1] + 1].tolist() == [sizes.get(L, 0) for L in range(lengths[0], lengths[-1] + 1)]
        want = chan.is_statement(3, 7, 8)
        assert (want[0][2:] >= 0).all() and want[1].max() > 8, m
        chan.is_statement(3, 3, 16)


def test_top_k_winners_scattered_over_lanes_waves_and_classes():
    """about 600 entries all one plain edit from a query, scattered among 1800 that are far: the winners are the K lowest
    original indices wherever they lie, `found` is the full count, ties are ordered by index, -1 fills"""
    rng = np.random.default_rng(53)
    V = 8
    q = word(rng, V, 9)
    ones = []
    for p in range(9):
        ones += [q[:p] + [v] + q[p + 1:] for v in range(V) if v != q[p]]
        ones.append(q[:p] + q[p + 1:])
        ones.append(q[:p] + [(q[p] + 3) % V] + q[p:])
    ones = [e for e in ones if e != q]
    far = lambda: [(v + 4) % V for v in q[:int(rng.integers(8, 11))]]
    rare = [(q[0] + 4) % V] * 12
    entries = [far() for _ in range(2400)]
    near_at = np.sort(rng.choice(len(entries), 600, replace=False))
    for i in near_at:
        entries[int(i)] = list(ones[int(rng.integers(0, len(ones)))])
    for i in np.setdiff1d(np.arange(len(entries)), near_at)[[5, 700, 1500]]:
        entries[int(i)] = rare[:-1] if i % 2 else rare + [1]
    chan = Chan(entries, [q, rare, word(rng, V, 30)], V, [([q[0], q[1]], [(q[0] + 4) % V] * 3, 90)], shuffle=rng)
    position = dict((int(e), p) for p, e in enumerate(chan.layout[1]))
    for K in (1, 8, 16):
        exact, found, cand, cost = chan.is_statement(50, 50, K)
        assert exact.tolist() == [-1, -1, -1] and found.tolist() == [600, 3, 0]
        assert cand[0].tolist() == near_at[:K].tolist() and (cost[0] == 50).all()
        assert (cand[1][:3] >= 0).all() and (cand[1][3:] == -1).all() and (cost[1][3:] == -1).all() and (cand[2] == -1).all()
    lanes = [position[int(e)] - int(chan.layout[2][len(entries[int(e)])]) for e in near_at[:16]]
    assert len(set(p % 64 for p in lanes)) > 8 and len(set(p // 64 % 4 for p in lanes)) == 4
    assert len(set(len(entries[int(e)]) for e in near_at[:16])) > 1
    exact, found, cand, cost = chan.is_statement(50, 100, 16)
    assert found[0] >= 600 and cand[0].tolist() == near_at[:16].tolist()


def test_ids_at_and_beyond_the_edges_of_the_table():
    """0 and V - 1 are ordinary ids; V, -1 and 2^31 - 1 equal nothing, themselves included, in queries, entries and rules -- a
    rule that holds one is ignored"""
    for V in (8, 4096):
        heads = [0, V - 1, V, -1, INT_MAX, 1]
        entries = [[h, 1, 2, V - 1, 0] for h in heads] + [[h] for h in heads] + [[2, 1, h, 1, 2] for h in heads]
        entries += [[INT_MAX] * 64, [-1] * 3, [V] * 2, [0] * 64, [V - 1] * 63, [V - 1, V - 1, 1, 2, V - 1, 0]]
        queries = [list(e) for e in entries] + [[V + 1, 1, 2, V - 1, 0], [-2 ** 31], [0] * 63 + [INT_MAX]]
        rules = [([0], [V - 1, V - 1], 3), ([V - 1, 0], [0], 4), ([V - 1], [], 5)]
        bad = [([V], [1], 0), ([1], [V], 0), ([-1], [1], 0), ([1], [-1], 0), ([INT_MAX], [0], 0), ([1, V], [1], 0), ([2], [1, 1, 1, INT_MAX], 0)]
        chan = Chan(entries, queries, V, rules + bad)
        exact, found, cand, cost = chan.is_statement(10, 20, 16)
        assert exact[:6].tolist() == [0, 1, -1, -1, -1, 5]
        assert reached((exact, found, cand, cost), 0, len(entries) - 1) == 3 and reached((exact, found, cand, cost), 2, 2) == 10
        good = Chan(entries, queries, V, rules)
        good.is_statement(10, 20, 16, want=(exact, found, cand, cost))      # (the ignored rules changed nothing)
        # rules whose lengths or costs are out of range, with garbage behind their used fields
        table, costs = records(rules)
        wild = np.array([[0, 1, 0, 0, 0, 0, 1, 0, 0, 0], [5, 0, 0, 0, 0, 0, 0, 0, 0, 0], [1, 5, 0, 0, 0, 0, 1, 1, 1, 1],
                         [-3, -3, 0, 0, 0, 0, 0, 0, 0, 0], [INT_MAX, 1, 0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                         [1, 0, 1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
        noisy = table.copy()
        for r in range(len(noisy)):
            noisy[r, 2 + noisy[r, 0]:6] = INT_MAX
            noisy[r, 6 + noisy[r, 1]:] = -1
        good.set_rules((np.concatenate([wild, noisy]), np.concatenate([np.array([0, 0, 0, 0, 0, -1, 4096], dtype=np.int32), costs])))
        good.is_statement(10, 20, 16, want=(exact, found, cand, cost))


def test_one_query_many_queries_and_a_second_call():
    rng = np.random.default_rng(54)
    for V in (8, 4096):
        entries = [word(rng, V, int(rng.integers(1, 12))) for _ in range(900)]
        queries = [mutate(rng, entries[int(rng.integers(0, len(entries)))], V, int(rng.integers(0, 3))) for _ in range(300)]
        rules = [(word(rng, V, int(rng.integers(1, 3))), word(rng, V, int(rng.integers(0, 3))), int(rng.integers(0, 20))) for _ in range(40)]
        rules += [(e[:2], e[2:4], 2) for e in entries[:40] if len(e) >= 4]
        chan = Chan(entries, queries, V, rules)
        want = chan.is_statement(12, 24, 8)
        first = [raw(t).copy() for t in chan.out]
        assert (want[0] >= 0).sum() > 30 and (want[1] > 0).sum() > 100
        assert chan.run(12, 24, 8) == 0 and all(np.array_equal(x, raw(t)) for x, t in zip(first, chan.out))
        one = Chan(entries, queries[:1], V, rules)
        one.is_statement(12, 24, 8)
        # fewer queries than the arrays hold: nothing behind Q, or Q * K, is written
        assert chan.run(12, 24, 8, Q=7) == 0 and chan.holds(want, Q=7)


def test_errors_return_before_any_launch():
    rng = np.random.default_rng(55)
    V = 8
    entries = [word(rng, V, int(rng.integers(1, 9))) for _ in range(200)]
    queries = [mutate(rng, entries[i], V, 1) for i in range(20)]
    chan = Chan(entries, queries, V, [([1], [2], 3), ([2, 3], [], 4)])
    cf = chan.class_first
    sizes = chan.lib.kl_lexicon_channel_workspace_bytes
    assert chan.n_ws % 8 == 0 and chan.n_ws == sizes(1, 1, 2) and sizes(1, 1, 0) < chan.n_ws < sizes(1, 1, 1024)
    down, short, late, none = cf.copy(), cf.copy(), cf.copy(), cf * 0
    down[5] = down[4] - 1 if down[4] > 0 else down[6] + 1
    short[65] += 1
    late[1] = 1
    cases = [dict(table=down), dict(table=short), dict(table=late), dict(table=none),
             dict(n_chars=len(chan.layout[0]) + 1), dict(V=0), dict(V=4097), dict(Q=0), dict(Q=2 ** 31),
             dict(n_q=2 ** 40 + 1), dict(n_chars=2 ** 40 + 1), dict(R=-1), dict(R=1025)]
    cases += [{name: None} for name in chan.NAMES + ("class_first", "ws")]
    cases += [dict(shift={name: 2}) for name in ("chars", "order", "q_pool", "rules", "rule_cost", "exact", "found", "cand", "cost")]
    cases += [dict(shift={name: 4}) for name in ("q_off", "class_first", "ws")]
    for case in cases:
        assert chan.run(10, 20, 8, **case) == KL_ERR_ARG, case
        assert chan.untouched(), case
    for unit, max_cost, K in ((0, 20, 8), (4096, 20, 8), (10, -1, 8), (10, 4096, 8), (10, 20, 0), (10, 20, 17)):
        assert chan.run(unit, max_cost, K, room=16) == KL_ERR_ARG and chan.untouched(), (unit, max_cost, K)
    assert chan.run(10, 20, 8, ws_bytes=chan.n_ws - 1) == KL_ERR_WORKSPACE and chan.untouched()
    # both rule pointers may be null with R == 0
    chan.set_rules([])
    assert chan.run(10, 20, 8, rules=None, rule_cost=None) == 0
    bare = [raw(t).copy() for t in chan.out]
    chan.is_statement(10, 20, 8)
    assert all(np.array_equal(x, raw(t)) for x, t in zip(bare, chan.out))
    chan.is_statement(4095, 4095, 16)


def test_without_rules_and_at_unit_one_it_is_kl_lexicon_neighbours():
    rng = np.random.default_rng(56)
    V = 5
    entries = [word(rng, V, int(rng.integers(1, 20))) for _ in range(700)] + [[1] * 64, [1] * 56, [2] * 9]
    queries = [mutate(rng, entries[int(rng.integers(0, len(entries)))], V, int(rng.integers(0, 4))) for _ in range(60)]
    queries += [[1] * 64, [1] * 60, [2], [], [3] * 65]
    look, chan = Look(entries, queries, V), Chan(entries, queries, V)
    for max_dist in (0, 1, 2, 5, 8):
        assert look.run(max_dist, 16) == 0 and chan.run(1, max_dist, 16) == 0
        for a, b in zip(look.out, chan.out):
            assert np.array_equal(raw(a), raw(b)), max_dist
    assert (look.out[1].cpu().numpy()[:len(queries)] > 16).any()


# ---------------------------------------------------------------------------------------------- engine and Rater
def test_engine_wrapper_and_rater_lexicon_neighbours_with_a_channel():
    from ocrd_keraslm_amd.lib import hipabi
    from tests.test_rater_golden import hip_factory
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 1)
    rng = np.random.default_rng(57)
    V = 20
    entries = [word(rng, V, int(rng.integers(1, 9))) for _ in range(500)]
    queries = [mutate(rng, entries[int(rng.integers(0, 500))], V, int(rng.integers(0, 3))) for _ in range(50)] + [[], [3] * 65]
    table, costs = records([(word(rng, V, int(rng.integers(1, 3))), word(rng, V, int(rng.integers(0, 3))), int(rng.integers(0, 9)))
                            for _ in range(30)])
    chars, order, class_first = ratebulk.lexicon_layout_host(*pooled(entries))
    q_pool, q_off = pooled(queries)
    want = ratebulk.lexicon_channel_host(q_pool, q_off, chars, order, class_first, V, table, costs, 7, 12, 5)
    good = dict(chars=up(chars), order=up(order), class_first=class_first, V=V, q_pool=up(q_pool), q_off=up(q_off), rules=up(table),
                rule_cost=up(costs), unit=7, max_cost=12, K=5)
    call = lambda a: lm.lexicon_channel(a["chars"], a["order"], a["class_first"], a["V"], a["q_pool"], a["q_off"], a["rules"],
                                        a["rule_cost"], a["unit"], a["max_cost"], a["K"])
    got = call(good)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got) and [tuple(t.shape) for t in got] == [(52,), (52,), (52, 5), (52, 5)]
    for g, r in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), r)
    bare = call(dict(good, rules=None, rule_cost=None))
    for g, r in zip(bare, ratebulk.lexicon_channel_host(q_pool, q_off, chars, order, class_first, V, None, None, 7, 12, 5)):
        assert np.array_equal(g.cpu().numpy(), r)
    for wrong in (dict(chars=up(chars).long()), dict(q_off=up(q_off).int()), dict(order=up(order)[::2]), dict(q_pool=torch.from_numpy(q_pool)),
                  dict(class_first=class_first[:-1]), dict(K=17), dict(unit=0), dict(unit=4096), dict(max_cost=4096), dict(V=4097),
                  dict(rules=up(table).long()), dict(rules=up(table)[:, :9]), dict(rules=up(table)[:-1]), dict(rule_cost=None),
                  dict(rules=None), dict(rule_cost=torch.from_numpy(costs)), dict(rules=up(table).reshape(-1)),
                  dict(rules=up(np.zeros((1025, 10), dtype=np.int32)), rule_cost=up(np.zeros(1025, dtype=np.int32)))):
        with pytest.raises(hipabi.KlError):
            call(dict(good, **wrong))
    # the Rater: normalised, unique, spread back over the duplicates; the device copy of the channel is made once
    hip = small_rater(hip_factory)
    assert hasattr(hip.model, "lexicon_channel")
    lex = hip.lexicon(lexicon_words(rng, 400))
    ch = hip.channel([("e", "c", 10, 40), ("h", "b", 5, 10), ("cf", "d", 3, 4), ("a", "", 2, 64), ("g", "ab", 7, 7)], unit_bits=6.0)
    words = lexicon_words(rng, 60) + [lex.words[9], "a?c", "", "ab" * 40]
    words += words[:9]
    near = hip.lexicon_neighbours(words, lex, per_word=6, channel=ch, max_bits=9.0)
    held = ch.on_device(hip.model)
    pool, off = pooled([[hip.mapping[0].get(c, 0) for c in w] for w in words])
    want = ratebulk.lexicon_channel_host(pool, off, lex.chars, lex.order, lex.class_first, hip.voc_size, ch.rules, ch.cost, 96, 144, 6)
    for g, r in zip((near.exact, near.found, near.index, near.dist), want):
        assert g.dtype == np.int32 and np.array_equal(g, r)
    assert near.exact[60] == 9 and near.found.max() > 6 and np.array_equal(near.bits[near.dist >= 0] * 16, near.dist[near.dist >= 0])
    again = hip.lexicon_neighbours(words[:5], lex, per_word=2, channel=ch, max_bits=3.0)
    assert all(a is b for a, b in zip(held, ch.on_device(hip.model))) and np.array_equal(again.exact, near.exact[:5])
    assert held[0].is_cuda and held[0].dtype == torch.int32 and tuple(held[0].shape) == (5, 10)
    none = hip.lexicon_neighbours([], lex, channel=ch)
    assert len(none) == 0 and none.index.shape == (0, 8)
    empty = hip.channel([], unit_bits=6.0)
    plain = hip.lexicon_neighbours(words, lex, per_word=6, channel=empty, max_bits=12.0)
    unit = hip.lexicon_neighbours(words, lex, per_word=6, max_dist=2)
    assert empty.on_device(hip.model) == (None, None) and np.array_equal(plain.index, unit.index)


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_rater_correct_words_with_a_channel_is_the_chain_by_hand(precision):
    """`suspect_words`, the weighted look-up, `word_edits`, `rescore(prior=..)`: the same words, the same edits, the same priors,
    and every field of the result identical to `rescore` called by hand -- it is the same code path; and the prior is what
    it says: the costs of the prior-less call plus the channel's bits, the choice `span_pick_host`'s over the sums, with a
    span at which it changes the winner"""
    from tests.test_rater_golden import hip_factory
    texts, contexts = contract_texts()
    rng = np.random.default_rng(58)
    texts = list(texts) + [random_text(rng, 30) for _ in range(3)]
    contexts = list(contexts) + [[175]] * 3
    hip = small_rater(hip_factory)
    lex, ch = channel_case(hip, rng, texts)
    rule = dict(k=2, streams=4, max_prob=1.0, min_rank=0, min_suspects=0)
    rescoring = dict(streams=4, left=12, ahead=3, min_gain=0.5)
    picks = {}
    for known, weight in ((False, 1.0), (True, 1.0), (False, 0.0), (False, 2.5)):
        found, rescored, bits = hip.correct_words(texts, lex, contexts, per_word=4, known=known, precision=precision, channel=ch,
                                                  max_bits=8.0, channel_weight=weight, **dict(rule, **rescoring))
        ref_found, edits, prior, ref_rescored, ref_bits = composed_channel(
            hip, texts, contexts, lex, ch, 8.0, 4, known, weight, dict(rule, precision=precision), dict(rescoring, precision=precision))
        assert np.array_equal(bits, ref_bits)
        for one, ref in zip(found, ref_found):
            assert one.spans() == ref.spans() and np.array_equal(one.bits, ref.bits)
        same_rescored(rescored, ref_rescored)
        assert sum(len(one) for one in rescored) == len(edits) > 3
        picks[known, weight] = np.concatenate([one.best for one in rescored])
    assert not np.array_equal(picks[False, 0.0], picks[False, 2.5])
    prior_is_added(hip, texts, edits, contexts, prior, dict(rescoring, precision=precision))
    assert winner_changes(hip, texts, lex, contexts, ch, dict(rule, precision=precision, **rescoring)) > 0
    assert hip.model.states.shape[0] == 1 and not hip.model.states.cpu().numpy().any()


def test_cli_lexicon_with_a_channel_on_the_device(tmp_path):
    from ocrd_keraslm_amd.scripts import run
    from tests.test_rater_golden import hip_factory
    model = str(tmp_path / "model.h5")
    small_rater(hip_factory).save(model)
    rng = np.random.default_rng(59)
    files, texts = [], []
    for i, size in enumerate((90, 70)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        texts.append(random_text(rng, size))
        name.write_text(texts[-1])
        files.append(str(name))
    ref = run._load(model)
    assert hasattr(ref.model, "lexicon_channel")
    lex, _ = channel_case(ref, rng, texts)
    listing = tmp_path / "words.tsv"
    listing.write_text("".join("%s\t%d\n" % (w, i) for i, w in enumerate(lex.words)))
    table = [("a", "b", 30, 60), ("c", "ef", 5, 50), ("gh", "d", 4, 8), ("b", "", 3, 90), ("e", "h", 2, 4)]
    counts = tmp_path / "counts.jsonl"
    counts.write_text("".join(json.dumps({"source": s, "target": t, "count": c, "occ": o, "rate": c / o}) + "\n" for s, t, c, o in table))
    res = CliRunner().invoke(run.cli, ["lexicon", "-m", model, "--lexicon", str(listing), "--apply", "-s", "4", "-k", "2", "--max-prob",
                                       "1", "--min-rank", "0", "--min-suspects", "0", "--per-word", "4", "--left", "10", "--ahead", "2",
                                       "--min-gain", "0.25", "--channel", str(counts), "--unit-bits", "7", "--max-bits", "8",
                                       "--channel-weight", "0.5"] + files)
    assert res.exit_code == 0, res.output + repr(res.exception)
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    assert [l["file"] for l in lines] == files
    ch = ref.channel(table, unit_bits=7.0)
    _, found, _ = ref.correct_words(texts, lex, [[170], [174]], per_word=4, k=2, max_prob=1.0, min_rank=0, min_suspects=0, left=10,
                                    ahead=2, min_gain=0.25, streams=4, channel=ch, max_bits=8.0, channel_weight=0.5)
    assert sum(int((f.best >= 0).sum()) for f in found) > 0
    for line, text, one in zip(lines, texts, found):
        assert type(one) is ratebatch.Rescored and line["chars"] == len(text) and line["corrected"] == one.apply(text)
        assert line["rescored"] == [[int(a), int(b), text[int(a):int(b)], new, float(g)]
                                    for a, b, new, g in zip(one.starts, one.ends, one.proposals(), one.gain)]
