"""Look-up across word boundaries on the GPU (run with -m gpu on an MI355X): kl_lexicon_splits, `HipLM.lexicon_splits`,
`Rater.lexicon_splits` and `Rater.correct_words(boundaries=True)`.

The kernel is held to its numpy statement (`ratebulk.lexicon_splits_host`, itself held to a brute force over all triples in
test_lexicon_splits.py) bit for bit: all five outputs are integers.  Every output byte is FILL before a call, and 64 elements
behind each output must keep it.  The shapes are the smallest at which the kernel can go wrong: query lengths at the edges of a
32- and a 64-bit pattern word, halves at the edges of the window the budget opens, length classes of a lane more and a lane less
than a wave and a round of the workgroup, winners of a split point's minimum scattered over lanes and waves."""
import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebulk
from tests.test_lexicon import pooled, same_rescored
from tests.test_lexicon_gpu import shuffled, word
from tests.test_lexicon_splits import ENTRIES, RESCORING, RULE, TEXTS, chain_by_hand
from tests.test_rate_bulk_gpu import device, lib_and_stream, small_rater
from tests.test_rate_window_gpu import make_model, ptr
from tests.test_rate_words_gpu import FILL, KL_ERR_ARG, KL_ERR_WORKSPACE, marked, raw, same_bytes, shifted, up

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
OUTPUTS = ("found", "split", "left", "right", "dist")


class Cut(object):
    """kl_lexicon_splits on device copies of a lexicon (entries: lists of ids, original index = place in the list) and of
    queries; five outputs of Q (Q * K) entries plus a guard band -- the pattern of test_lexicon_gpu.Look"""
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
        self.n_ws = self.lib.kl_lexicon_splits_workspace_bytes(self.Q, 16)
        self.ws = self.torch.full((max(self.n_ws, 8),), FILL, dtype=self.torch.uint8, device=self.dev)

    def want(self, max_dist, min_part, K):
        return ratebulk.lexicon_splits_host(*self.queries, *self.layout, V=self.V, max_dist=max_dist, min_part=min_part, K=K)

    def run(self, max_dist, min_part, K, room=None, ws_bytes=None, shift=None, table=None, **override):
        torch = self.torch
        room = K if room is None else room
        self.out = [marked(self.Q, torch.int32)] + [marked(self.Q * room, torch.int32) for _ in range(4)]
        self.ws.fill_(FILL)
        cf = self.class_first if table is None else np.ascontiguousarray(table, dtype=np.int64)      # (on the host)
        a = dict(zip(self.NAMES, [ptr(t) for t in self.src] + [ptr(t) for t in self.out]), n_chars=len(self.layout[0]), V=self.V,
                 n_q=len(self.queries[0]), Q=self.Q, class_first=ptr(torch.from_numpy(cf)), ws=ptr(self.ws))
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_lexicon_splits(a["chars"], a["n_chars"], a["order"], a["class_first"], a["V"], a["q_pool"], a["n_q"],
                                          a["q_off"], a["Q"], max_dist, min_part, K, a["found"], a["split"], a["left"], a["right"],
                                          a["dist"], a["ws"], self.n_ws if ws_bytes is None else ws_bytes, self.stream)
        torch.cuda.synchronize()
        return code

    def holds(self, want, Q=None):
        """the outputs are want's for the first Q queries, bit for bit, and everything behind keeps FILL"""
        Q = self.Q if Q is None else Q
        return all(same_bytes(t, np.ascontiguousarray(w).reshape(-1), Q * (w.size // max(len(w), 1)))
                   for t, w in zip(self.out, want))

    def is_statement(self, max_dist, min_part, K):
        want = self.want(max_dist, min_part, K)
        assert self.run(max_dist, min_part, K) == 0
        for t, w, name in zip(self.out, want, OUTPUTS):
            assert same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size), (name, max_dist, min_part, K)
        return want

    def untouched(self):
        return all((raw(t) == FILL).all() for t in self.out) and (raw(self.ws) == FILL).all()


def other(rng, V, not_this):
    return int((not_this + 1 + rng.integers(0, V - 1)) % V)


def longer(rng, V, half, n):
    """the half with n ids inserted, none of them equal to a neighbour: n edits away and no fewer"""
    half = list(half)
    for _ in range(n):
        at = int(rng.integers(0, len(half) + 1))
        near = set(half[max(at - 1, 0):at + 1])
        half.insert(at, [v for v in range(V) if v not in near][int(rng.integers(0, V - len(near)))])
    return half


LENGTHS = (2, 3, 31, 32, 33, 63, 64)


def lengths_case():
    """queries of 2, 3, 31, 32, 33, 63 and 64 ids (and of 0, 1 and 65); per query and for the split points 1, m // 2 and m - 1
    both halves as entries, the halves with a substitution at their first and at their last id, and a left half with d = 1 ids
    more, with d ids fewer and with d + 1 ids more -- at the edge of the window max_dist 2 opens and outside it"""
    rng = np.random.default_rng(30)
    V = 8
    queries, entries, marks = [], [], {}
    for m in LENGTHS:
        q = word(rng, V, m)
        queries.append(q)
        for s in sorted(set((1, m // 2, m - 1))):
            a, b = q[:s], q[s:]
            marks[m, s] = len(entries)
            entries += [list(a), list(b), [other(rng, V, a[0])] + a[1:], b[:-1] + [other(rng, V, b[-1])]]
            entries += [longer(rng, V, a, 1), longer(rng, V, a, 2), a[1:], longer(rng, V, b, 1), b[:-1]]      # (no ids: left out)
        entries += [word(rng, V, max(1, min(64, m // 2 + int(rng.integers(-3, 4))))) for _ in range(6)]
    queries += [[], word(rng, V, 1), word(rng, V, 65)]
    return V, entries, queries, marks


@pytest.mark.parametrize("narrow", ["1", "0"])
def test_query_lengths_at_the_edges_of_the_pattern_word_and_halves_at_the_edges_of_the_window(narrow, monkeypatch):
    """(narrow 1, the default: queries of at most 32 ids run on a 32-bit pattern word; KL_LEXICON_NARROW=0: all on 64 bits)"""
    monkeypatch.setenv("KL_LEXICON_NARROW", narrow)
    V, entries, queries, marks = lengths_case()
    cut = Cut(entries, queries, V)
    # max_dist 1: the halves must be exact
    found, split, left, right, dist = cut.is_statement(1, 1, 16)
    for row, m in enumerate(LENGTHS):
        for s in sorted(set((1, m // 2, m - 1))):
            assert s in split[row].tolist() or found[row] > 16, (m, s)
            if s in split[row].tolist():
                at = split[row].tolist().index(s)
                assert entries[left[row, at]] == queries[row][:s] and entries[right[row, at]] == queries[row][s:]
                assert left[row, at] <= marks[m, s] and dist[row, at] == 1
    assert found[-3:].tolist() == [0, 0, 0] and all((a[-3:] == -1).all() for a in (split, left, right, dist))
    # max_dist 2: a half one id longer or shorter is within the window, the total is 2 where a half is not exact
    found2, split2, left2, right2, dist2 = cut.is_statement(2, 1, 16)
    assert (found2 >= found).all() and (found2 > found).any() and set(dist2.reshape(-1).tolist()) == {-1, 1, 2}
    cut.is_statement(2, 2, 4)
    # min_part larger than half of the shorter queries; the whole budget
    found, split, left, right, dist = cut.is_statement(3, 17, 16)
    assert found[:4].tolist() == [0, 0, 0, 0] and (split[:4] == -1).all() and found[4:7].max() > 0
    cut.is_statement(8, 1, 16)
    cut.is_statement(8, 32, 2)


def test_halves_at_s_minus_d_s_plus_d_and_one_beyond():
    """one query, one split point s, d = 2: entries for the left half of s - d, s + d and s + d + 1 ids, each alone in its
    lexicon beside the exact right half -- the first two make the split, the third lies outside the window and must not;
    the same for the right half; and both halves at d is beyond the budget of the whole"""
    rng = np.random.default_rng(31)
    V = 6
    for m, s in ((12, 5), (40, 33), (64, 32)):
        q = word(rng, V, m)
        a, b = q[:s], q[s:]
        for side, (half, whole) in enumerate(((a, b), (b, a))):
            for change, total in ((half[2:], 3), (longer(rng, V, half, 2), 3), (longer(rng, V, half, 3), None)):
                entries = [list(whole), change] + [word(rng, V, 64) for _ in range(3)]
                cut = Cut(entries, [q], V)
                found, split, left, right, dist = cut.is_statement(3, 3, 2)
                if total is None:
                    assert found[0] == 0 or s not in split[0].tolist(), (m, s, side)
                else:
                    at = split[0].tolist().index(s)
                    assert (left[0, at], right[0, at], dist[0, at]) == ((1, 0, 3) if side == 0 else (0, 1, 3)), (m, s, side)
        cut = Cut([a[2:], b[:-2]], [q], V)
        assert cut.is_statement(3, 3, 2)[0][0] == 0 and cut.is_statement(5, 3, 2)[0][0] >= 1


def classes_case():
    """length classes of 63, 64, 65, 255, 256 and 257 entries (and one of 700), shuffled within; the queries are two entries
    run together, so that the winner of a split point comes from any lane and wave, and every entry has twins at scattered
    indices, so that the least index must win"""
    rng = np.random.default_rng(32)
    V = 3
    sizes = {2: 63, 3: 64, 4: 65, 5: 255, 6: 256, 7: 257, 8: 700}
    entries = [word(rng, V, L) for L, n in sizes.items() for _ in range(n)]
    entries = [entries[i] for i in rng.permutation(len(entries))]
    pick = lambda L, which: entries[int(np.nonzero([len(e) == L for e in entries])[0][which])]
    queries = [pick(L, -1) + pick(M, -1) for L in sizes for M in (2, 5, 8)]      # the last lanes of the classes
    queries += [pick(L, int(rng.integers(0, n))) + pick(9 - L if L < 8 else 8, 0) for L, n in sizes.items()]
    queries += [word(rng, V, int(rng.integers(4, 17))) for _ in range(12)]
    return V, sizes, entries, queries


def test_class_sizes_across_a_wave_and_a_round_of_the_workgroup():
    V, sizes, entries, queries = classes_case()
    cut = Cut(entries, queries, V, shuffle=np.random.default_rng(33))
    assert np.diff(cut.layout[2])[2:9].tolist() == list(sizes.values())
    found, split, left, right, dist = cut.is_statement(1, 2, 8)
    assert (found[:len(queries) - 12] >= 1).all() and found.max() > 1
    # twins: the index named is the least of the identical entries
    first = {}
    for i, e in enumerate(entries):
        first.setdefault(tuple(e), i)
    named = [(int(i), entries[int(i)]) for i in np.concatenate([left.reshape(-1), right.reshape(-1)]) if i >= 0]
    assert all(first[tuple(e)] == i for i, e in named) and len(set(i for i, _ in named)) > 40
    position = dict((int(e), p) for p, e in enumerate(cut.layout[1]))
    lanes = [position[i] - int(cut.layout[2][len(e)]) for i, e in named]
    assert len(set(p % 64 for p in lanes)) > 32 and len(set(p // 64 % 4 for p in lanes)) == 4      # lanes, and all four waves
    found, split, left, right, dist = cut.is_statement(3, 2, 16)
    assert set(dist.reshape(-1).tolist()) == {-1, 1, 2, 3} and found.max() >= 8
    cut.is_statement(2, 1, 3)


def test_selection_below_at_and_above_the_number_of_places_and_ties_decided_by_s():
    """`abab..` over the entries ab, abab, ..: every even place is a split into two entries, and pairs of places share their
    larger index -- (ab, ababab) and (ababab, ab) -- so that s decides; a query of 64 ids has 31 places"""
    V = 4
    entries = [[0, 1] * n for n in range(1, 33)] + [[2, 3]]
    queries = [[0, 1] * 4, [0, 1] * 32, [0, 1] * 4 + [2], [2, 3, 2, 3], [0, 1, 2, 3]]
    cut = Cut(entries, queries, V)
    for K in (1, 2, 3, 4, 16):
        found, split, left, right, dist = cut.is_statement(1, 1, K)
        assert found.tolist() == [3, 31, 0, 1, 1]
        assert split[0].tolist() == ([4, 2, 6] + [-1] * 13)[:K] and left[0].tolist() == ([1, 0, 2] + [-1] * 13)[:K]
        assert split[1, 0] == 32 and (K < 3 or split[1, 1:3].tolist() == [30, 34])
    found, split, left, right, dist = cut.is_statement(2, 1, 16)
    assert found.tolist() == [3, 31, 4, 1, 1] and dist[2, :4].tolist() == [2, 2, 2, 2] and split[2, :4].tolist() == [4, 2, 6, 8]


def test_ids_outside_the_table_two_calls_and_fewer_queries():
    """V, -1 and 2^31 - 1 equal nothing, themselves included, and never index the table; a second call gives the same bytes;
    nothing behind Q, or Q * K, is written"""
    rng = np.random.default_rng(34)
    for V in (8, 4096):
        odd = [V, -1, INT_MAX, 0, V - 1]
        entries = [[h, 1, 2] for h in odd] + [[2, 1, h] for h in odd] + [[h] for h in odd] + [word(rng, V, int(rng.integers(1, 7))) for _ in range(300)]
        queries = [entries[int(a)] + entries[int(b)] for a, b in rng.integers(0, len(entries), (60, 2))]
        queries += [[V, 1, 2, 2, 1, V], [0, 1, 2, V - 1, 1, 2], [-2 ** 31, 3], [INT_MAX] * 64]
        cut = Cut(entries, queries, V, shuffle=rng)
        want = cut.is_statement(2, 1, 4)
        first = [raw(t).copy() for t in cut.out]
        assert (want[0] > 0).sum() > 40 and want[0][-4:].tolist()[1] >= 1 and want[4][-4, 0] in (-1, 2)
        assert cut.run(2, 1, 4) == 0 and all(np.array_equal(x, raw(t)) for x, t in zip(first, cut.out))
        assert cut.run(2, 1, 4, Q=7) == 0 and cut.holds(want, Q=7)
        Cut(entries, queries[:1], V).is_statement(2, 1, 4)


def test_errors_return_before_any_launch():
    rng = np.random.default_rng(35)
    V = 8
    entries = [word(rng, V, int(rng.integers(1, 9))) for _ in range(200)]
    queries = [entries[i] + entries[i + 1] for i in range(20)]
    cut = Cut(entries, queries, V)
    cf = cut.class_first
    assert cut.n_ws % 8 == 0 and cut.n_ws == cut.lib.kl_lexicon_splits_workspace_bytes(1, 1)
    down, short, late, none = cf.copy(), cf.copy(), cf.copy(), cf * 0
    down[5] = down[4] - 1 if down[4] > 0 else down[6] + 1          # decreases
    short[65] += 1                                                   # one entry more than n_chars holds ids for
    late[1] = 1                                                      # class_first[1] != 0
    cases = [dict(table=down), dict(table=short), dict(table=late), dict(table=none),
             dict(n_chars=len(cut.layout[0]) + 1), dict(V=0), dict(V=4097), dict(Q=0), dict(Q=2 ** 31),
             dict(n_q=2 ** 40 + 1), dict(n_chars=2 ** 40 + 1)]
    cases += [{name: None} for name in cut.NAMES + ("class_first", "ws")]
    cases += [dict(shift={name: 2}) for name in ("chars", "order", "q_pool") + OUTPUTS]
    cases += [dict(shift={name: 4}) for name in ("q_off", "class_first", "ws")]
    for case in cases:
        assert cut.run(2, 2, 8, **case) == KL_ERR_ARG, case
        assert cut.untouched(), case
    for max_dist, min_part, K in ((0, 2, 8), (-1, 2, 8), (9, 2, 8), (2, 0, 8), (2, -1, 8), (2, 33, 8), (2, 2, 0), (2, 2, 17)):
        assert cut.run(max_dist, min_part, K, room=16) == KL_ERR_ARG and cut.untouched(), (max_dist, min_part, K)
    assert cut.run(2, 2, 8, ws_bytes=cut.n_ws - 1) == KL_ERR_WORKSPACE and cut.untouched()
    assert cut.is_statement(2, 2, 8)[0].max() >= 1
    cut.is_statement(8, 1, 16)


# ---------------------------------------------------------------------------------------------- engine and Rater
def test_engine_wrapper_and_rater_lexicon_splits():
    from ocrd_keraslm_amd.lib import hipabi
    from tests.test_rater_golden import hip_factory
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 1)
    rng = np.random.default_rng(36)
    V = 20
    entries = [word(rng, V, int(rng.integers(1, 7))) for _ in range(500)]
    queries = [entries[int(a)] + entries[int(b)] for a, b in rng.integers(0, 500, (50, 2))] + [[], [3] * 65]
    chars, order, class_first = ratebulk.lexicon_layout_host(*pooled(entries))
    q_pool, q_off = pooled(queries)
    want = ratebulk.lexicon_splits_host(q_pool, q_off, chars, order, class_first, V, 2, 2, 5)
    got = lm.lexicon_splits(up(chars), up(order), class_first, V, up(q_pool), up(q_off), 2, 2, 5)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got) and [tuple(t.shape) for t in got] == [(52,)] + [(52, 5)] * 4
    for g, r in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), r)
    for wrong in (dict(chars=up(chars).long()), dict(q_off=up(q_off).int()), dict(order=up(order)[::2]), dict(q_pool=torch.from_numpy(q_pool)),
                  dict(class_first=class_first[:-1]), dict(K=17), dict(max_dist=0), dict(max_dist=9), dict(min_part=0), dict(min_part=33),
                  dict(V=4097)):
        a = dict(dict(chars=up(chars), order=up(order), class_first=class_first, V=V, q_pool=up(q_pool), q_off=up(q_off), max_dist=2,
                      min_part=2, K=5), **wrong)
        with pytest.raises(hipabi.KlError):
            lm.lexicon_splits(a["chars"], a["order"], a["class_first"], a["V"], a["q_pool"], a["q_off"], a["max_dist"], a["min_part"], a["K"])
    # the Rater: normalised, unique, spread back over the duplicates; the device copy of the lexicon is made once
    hip = small_rater(hip_factory)
    assert hasattr(hip.model, "lexicon_splits")
    lex = hip.lexicon(ENTRIES)
    words = ["badcab", "bad", "gagcafe", "", "hxadfee", "badcab", "a?cab", "ab" * 40, "aa", "facedeaf", "beadfeed"]
    splits = hip.lexicon_splits(words, lex, max_dist=2, min_part=1, per_word=3)
    held = lex.on_device(hip.model)
    pool, off = pooled([[hip.mapping[0].get(c, 0) for c in w] for w in words])
    want = ratebulk.lexicon_splits_host(pool, off, lex.chars, lex.order, lex.class_first, hip.voc_size, 2, 1, 3)
    for g, r in zip((splits.found, splits.at, splits.left, splits.right, splits.dist), want):
        assert g.dtype == np.int32 and np.array_equal(g, r)
    assert splits.strings(0)[0] == "bad cab" == splits.strings(5)[0] and splits.strings(4)[0] == "head fee"
    again = hip.lexicon_splits(words[:3], lex, per_word=2)
    assert all(a is b for a, b in zip(held, lex.on_device(hip.model))) and again.strings(0) == ["bad cab"]
    none = hip.lexicon_splits([], lex)
    assert len(none) == 0 and none.at.shape == (0, 4)


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_rater_correct_words_with_boundaries_is_the_chain_with_the_host_statements(precision):
    """texts with planted run-together and split words: the same edits, candidates, choices and costs as the chain written
    out by hand in test_lexicon_splits.py, whose three look-ups are the numpy statements -- rating and rescoring are the
    same device code on both sides, so the costs are identical, as in test_lexicon_gpu's composed call"""
    from tests.test_rater_golden import hip_factory
    hip = small_rater(hip_factory)
    assert hasattr(hip.model, "lexicon_splits") and hasattr(hip.model, "lexicon_neighbours")
    lex = hip.lexicon(ENTRIES)
    contexts = [[170 + i] for i in range(len(TEXTS))]
    for known, max_dist, min_part in ((False, 1, 2), (True, 2, 1)):
        found, rescored, bits = hip.correct_words(TEXTS, lex, contexts, max_dist=max_dist, per_word=4, known=known, boundaries=True,
                                                  min_part=min_part, precision=precision, **dict(RULE, **RESCORING))
        ref_found, edits, ref_rescored, ref_bits = chain_by_hand(hip, TEXTS, contexts, lex, max_dist, 4, known, min_part,
                                                                 dict(RULE, precision=precision), dict(RESCORING, precision=precision))
        assert np.array_equal(bits, ref_bits)
        for one, ref in zip(found, ref_found):
            assert one.spans() == ref.spans() and np.array_equal(one.bits, ref.bits)
        same_rescored(rescored, ref_rescored)
        by_span = dict(((i, a, b), c) for i, a, b, c in edits)
        assert "bad cab" in by_span[0, 2, 8] and by_span[0, 9, 15][0] == "ahead" and by_span[3, 6, 11][0] == "head"
        assert sum(len(one) for one in rescored) == len(edits) > 0 and sum(int((one.best >= 0).sum()) for one in rescored) > 0
    assert hip.model.states.shape[0] == 1 and not hip.model.states.cpu().numpy().any()
