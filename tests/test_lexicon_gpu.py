"""The lexicon look-up on the GPU (run with -m gpu on an MI355X): kl_lexicon_neighbours, `HipLM.lexicon_neighbours`,
`Rater.lexicon_neighbours`, `Rater.correct_words` and `keraslm-rate lexicon`.

The kernel is held to its numpy statement (`ratebulk.lexicon_neighbours_host`, itself held to a two-row Levenshtein distance in
test_lexicon.py) bit for bit: all four outputs are integers.  Every output byte is FILL before a call, and 64 elements behind
each output must keep it.  The shapes are the smallest at which the kernel can go wrong: query lengths at the edges of a 32- and
a 64-bit pattern word, length classes at the edge of the window max_dist opens, classes of a lane more and a lane less than a
wave and a round of the workgroup, winners of the top-K merge scattered over lanes and waves."""
import json

import numpy as np
import pytest
from click.testing import CliRunner

from ocrd_keraslm_amd.lib import ratebatch, ratebulk
from tests.test_lexicon import brute_neighbours, composed, lev, lexicon_words, mutate, pooled, same_rescored
from tests.test_rate_bulk_gpu import device, lib_and_stream, random_text, small_rater
from tests.test_rate_suspects import contract_texts
from tests.test_rate_window_gpu import make_model, ptr
from tests.test_rate_words_gpu import FILL, KL_ERR_ARG, KL_ERR_WORKSPACE, marked, raw, same_bytes, shifted, up

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


class Look(object):
    """kl_lexicon_neighbours on device copies of a lexicon (entries: lists of ids, original index = place in the list) and of
    queries; four outputs of Q (Q * K) entries plus a guard band"""
    NAMES = ("chars", "order", "q_pool", "q_off", "exact", "found", "cand", "dist")

    def __init__(self, entries, queries, V, shuffle=None):
        self.torch, self.dev = device()
        self.lib, self.stream = lib_and_stream()
        self.V, self.Q = V, len(queries)
        self.layout = shuffled(ratebulk.lexicon_layout_host(*pooled(entries)), shuffle)
        self.queries = pooled(queries)
        some = lambda a: up(a) if len(a) else self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)
        self.src = [some(self.layout[0]), some(self.layout[1]), some(self.queries[0]), up(self.queries[1])]
        self.class_first = np.ascontiguousarray(self.layout[2])
        self.n_ws = self.lib.kl_lexicon_neighbours_workspace_bytes(self.Q, 16)
        self.ws = self.torch.full((max(self.n_ws, 8),), FILL, dtype=self.torch.uint8, device=self.dev)

    def want(self, max_dist, K):
        return ratebulk.lexicon_neighbours_host(*self.queries, *self.layout, V=self.V, max_dist=max_dist, K=K)

    def run(self, max_dist, K, room=None, ws_bytes=None, shift=None, table=None, **override):
        torch = self.torch
        room = K if room is None else room
        self.out = [marked(self.Q, torch.int32), marked(self.Q, torch.int32), marked(self.Q * room, torch.int32),
                    marked(self.Q * room, torch.int32)]
        self.ws.fill_(FILL)
        cf = self.class_first if table is None else np.ascontiguousarray(table, dtype=np.int64)      # (on the host)
        a = dict(zip(self.NAMES, [ptr(t) for t in self.src] + [ptr(t) for t in self.out]), n_chars=len(self.layout[0]), V=self.V,
                 n_q=len(self.queries[0]), Q=self.Q, class_first=ptr(torch.from_numpy(cf)), ws=ptr(self.ws))
        a.update(override)
        for name, by in (shift or {}).items():
            a[name] = shifted(a[name], by)
        code = self.lib.kl_lexicon_neighbours(a["chars"], a["n_chars"], a["order"], a["class_first"], a["V"], a["q_pool"], a["n_q"],
                                              a["q_off"], a["Q"], max_dist, K, a["exact"], a["found"], a["cand"], a["dist"],
                                              a["ws"], self.n_ws if ws_bytes is None else ws_bytes, self.stream)
        torch.cuda.synchronize()
        return code

    def holds(self, want, Q=None):
        """the outputs are want's for the first Q queries, bit for bit, and everything behind keeps FILL"""
        Q = self.Q if Q is None else Q
        return all(same_bytes(t, np.ascontiguousarray(w).reshape(-1), Q * (w.size // max(len(w), 1)))
                   for t, w in zip(self.out, want))

    def is_statement(self, max_dist, K):
        want = self.want(max_dist, K)
        assert self.run(max_dist, K) == 0
        for t, w, name in zip(self.out, want, ("exact", "found", "cand", "dist")):
            assert same_bytes(t, np.ascontiguousarray(w).reshape(-1), w.size), (name, max_dist, K)
        return want

    def untouched(self):
        return all((raw(t) == FILL).all() for t in self.out) and (raw(self.ws) == FILL).all()


def shuffled(layout, rng):
    """the layout with the entries of every length class in a random order (None: as it is) -- at the level of the C ABI
    `order` is any list of indices, and an entry's place within its class decides which lane walks it"""
    if rng is None:
        return layout
    chars, order, class_first = (a.copy() for a in layout)
    base = 0
    for L in range(1, 65):
        a, b = int(class_first[L]), int(class_first[L + 1])
        perm = rng.permutation(b - a)
        order[a:b] = order[a:b][perm]
        chars[base:base + L * (b - a)] = chars[base:base + L * (b - a)].reshape(L, b - a)[:, perm].reshape(-1)
        base += L * (b - a)
    return chars, order, class_first


def word(rng, V, n):
    return rng.integers(0, V, n).tolist()


@pytest.mark.parametrize("narrow", ["1", "0"])
def test_query_lengths_at_the_edges_of_the_pattern_word_and_of_the_class_window(narrow, monkeypatch):
    """(narrow 1, the default: queries of at most 32 ids run on a 32-bit pattern word; KL_LEXICON_NARROW=0: all on 64 bits)
    queries of 1, 2, 31, 32, 33, 63, 64 ids (and of 0 and 65) with max_dist 2, so that the class window clamps at 1 and at
    64; per query: itself, a substitution at its first and at its last id (the top bit carries the score), pure insertions
    and pure deletions of 1, 2 and 3 ids -- distance max_dist lies at the edge of the window, max_dist + 1 outside"""
    monkeypatch.setenv("KL_LEXICON_NARROW", narrow)
    rng = np.random.default_rng(10)
    V = 8
    queries, entries, marks = [], [], {}
    for m in (1, 2, 31, 32, 33, 63, 64):
        q = word(rng, V, m)
        queries.append(q)
        first = len(entries)
        entries.append(list(q))
        entries.append([(q[0] + 1) % V] + q[1:])
        entries.append(q[:-1] + [(q[-1] + 1) % V])
        for d in (1, 2, 3):
            longer = list(q)
            for _ in range(d):
                longer.insert(int(rng.integers(0, len(longer) + 1)), int(rng.integers(0, V)))
            entries.append(longer)                                  # (65 and more ids: left out of the layout)
            shorter = list(q)
            for _ in range(min(d, m)):
                del shorter[int(rng.integers(0, len(shorter)))]
            entries.append(shorter)                                 # (no ids: left out)
        marks[m] = first
        entries += [word(rng, V, max(1, min(64, m + int(rng.integers(-3, 4))))) for _ in range(6)]
    queries += [[], word(rng, V, 65)]
    look = Look(entries, queries, V)
    exact, found, cand, dist = look.is_statement(2, 16)
    for row, m in enumerate((1, 2, 31, 32, 33, 63, 64)):
        at, q = marks[m], queries[row]
        assert exact[row] == at, m
        # the pairs are what they are meant to be: substitutions at distance 1, d insertions or deletions at distance d ...
        expect = {at + 1: 1, at + 2: 1}
        for d in (1, 2, 3):
            expect.update({at + 1 + 2 * d: d, at + 2 + 2 * d: d})
        expect = dict((e, d) for e, d in expect.items() if 1 <= len(entries[e]) <= 64 and entries[e] != q)
        assert all(lev(q, entries[e], V) == d for e, d in expect.items()), m
        # ... and are listed with that distance up to max_dist, not beyond (a short query has more neighbours than places)
        assert found[row] <= 16 or m <= 2, m
        near = dict(zip(cand[row].tolist(), dist[row].tolist()))
        if found[row] <= 16:
            assert all((near.get(e) == d) == (d <= 2) for e, d in expect.items()), m
    assert exact[-2:].tolist() == [-1, -1] and found[-2:].tolist() == [0, 0] and (cand[-2:] == -1).all() and (dist[-2:] == -1).all()
    look.is_statement(0, 1)
    look.is_statement(8, 8)


def test_class_sizes_across_a_wave_and_a_round_of_the_workgroup():
    rng = np.random.default_rng(11)
    V = 3
    sizes = {3: 1, 4: 63, 5: 64, 6: 65, 7: 255, 8: 256, 9: 257, 10: 600}
    entries = [word(rng, V, L) for L, n in sizes.items() for _ in range(n)]
    entries = [entries[i] for i in rng.permutation(len(entries))]
    queries = [mutate(rng, entries[int(rng.integers(0, len(entries)))], V, int(rng.integers(0, 3))) for _ in range(36)]
    queries += [entries[int(np.nonzero([len(e) == L for e in entries])[0][-1])] for L in sizes]      # the last lane of every class
    look = Look(entries, queries, V)
    assert np.diff(look.layout[2])[3:11].tolist() == list(sizes.values())
    want = look.is_statement(2, 8)
    assert (want[0][-8:] >= 0).all() and want[1].max() > 16 and len(set(want[3].reshape(-1).tolist())) == 3
    look.is_statement(1, 16)


def test_top_k_winners_scattered_over_lanes_and_waves():
    """about 600 entries all at distance 1 from one query -- repeated and distinct ones, of the query's length and of one id
    more and less --, scattered among 1800 entries that are far: the winners are the K lowest original indices, wherever
    in their classes they lie; `found` is
    the full count; a query with fewer than K matches gets the -1 fill, a query with none nothing but it"""
    rng = np.random.default_rng(12)
    V = 8
    q = word(rng, V, 9)
    ones = []
    for p in range(9):
        ones += [q[:p] + [v] + q[p + 1:] for v in range(V) if v != q[p]]      # 63 distinct substitutions
        ones.append(q[:p] + q[p + 1:])
        ones.append(q[:p] + [(q[p] + 3) % V] + q[p:])
    far = lambda: [(v + 4) % V for v in q[:int(rng.integers(8, 11))]]
    rare = [(q[0] + 4) % V] * 12                                    # three entries within one edit of it, no more
    entries = [far() for _ in range(2400)]
    near_at = np.sort(rng.choice(len(entries), 600, replace=False))
    for i in near_at:
        entries[int(i)] = list(ones[int(rng.integers(0, len(ones)))])
    assert all(brute_neighbours([q], [e], V, 1, 1)[1][0] == 1 for e in ones)
    for i in np.setdiff1d(np.arange(len(entries)), near_at)[[5, 700, 1500]]:
        entries[int(i)] = rare[:-1] if i % 2 else rare + [1]
    look = Look(entries, [q, rare, word(rng, V, 30)], V, shuffle=rng)
    position = dict((int(e), p) for p, e in enumerate(look.layout[1]))
    for K in (1, 8, 16):
        exact, found, cand, dist = look.is_statement(1, K)
        assert exact.tolist() == [-1, -1, -1] and found.tolist() == [600, 3, 0]
        assert cand[0].tolist() == near_at[:K].tolist() and (dist[0] == 1).all()
        assert (cand[1][:3] >= 0).all() and (cand[1][3:] == -1).all() and (dist[1][3:] == -1).all() and (cand[2] == -1).all()
    lanes = [position[int(e)] - int(look.layout[2][len(entries[int(e)])]) for e in near_at[:16]]
    assert len(set(p % 64 for p in lanes)) > 8 and len(set(p // 64 % 4 for p in lanes)) == 4      # lanes, and all four waves
    assert len(set(len(entries[int(e)]) for e in near_at[:16])) > 1                                # more than one class
    # the order is (distance, index): with max_dist 2 the far-off index of a nearer entry still comes first
    exact, found, cand, dist = look.is_statement(2, 16)
    assert found[0] >= 600 and cand[0].tolist() == near_at[:16].tolist()


def test_exact_is_the_smallest_index_and_no_neighbour():
    rng = np.random.default_rng(13)
    V = 5
    entries = [word(rng, V, int(rng.integers(2, 7))) for _ in range(700)]
    twins = [3, 130, 131, 400, 699]
    for i in twins[1:]:
        entries[i] = list(entries[3])
    queries = [list(entries[3]), list(entries[500]), mutate(rng, entries[7], V, 1)] + [list(e) for e in entries[600:620]]
    look = Look(entries, queries, V)
    exact, found, cand, dist = look.is_statement(2, 16)
    assert exact[0] == 3 and not set(cand[0].tolist()) & set(twins) and (dist[dist >= 0] >= 1).all()
    exact, found, cand, dist = look.is_statement(0, 4)
    assert exact[0] == 3 and exact[1] >= 0 and not found.any() and (cand == -1).all() and (dist == -1).all()


def test_ids_at_and_beyond_the_edges_of_the_table():
    """0 and V - 1 are ordinary ids; V, -1 and 2^31 - 1 equal nothing, themselves included -- and never index the table"""
    for V in (8, 4096):
        heads = [0, V - 1, V, -1, INT_MAX, 1]
        entries = [[h, 1, 2, V - 1, 0] for h in heads] + [[h] for h in heads] + [[2, 1, h, 1, 2] for h in heads]
        entries += [[INT_MAX] * 64, [-1] * 3, [V] * 2, [0] * 64, [V - 1] * 63]
        queries = [list(e) for e in entries] + [[V + 1, 1, 2, V - 1, 0], [-2 ** 31], [0] * 63 + [INT_MAX]]
        look = Look(entries, queries, V)
        exact, found, cand, dist = look.is_statement(2, 16)
        assert exact[:6].tolist() == [0, 1, -1, -1, -1, 5]          # an id outside [0, V) is not even equal to itself
        near = dict(zip(cand[2].tolist(), dist[2].tolist()))
        assert near[2] == 1 and near[0] == 1 and near[4] == 1       # [V, ..] is one substitution away from its own entry
        look.is_statement(0, 1)


def test_one_query_many_queries_and_a_second_call():
    rng = np.random.default_rng(14)
    for V in (8, 4096):
        entries = [word(rng, V, int(rng.integers(1, 12))) for _ in range(900)]
        queries = [mutate(rng, entries[int(rng.integers(0, len(entries)))], V, int(rng.integers(0, 3))) for _ in range(300)]
        look = Look(entries, queries, V)
        want = look.is_statement(2, 8)
        first = [raw(t).copy() for t in look.out]
        assert (want[0] >= 0).sum() > 30 and (want[1] > 0).sum() > 100
        assert look.run(2, 8) == 0 and all(np.array_equal(x, raw(t)) for x, t in zip(first, look.out))
        one = Look(entries, queries[:1], V)
        one.is_statement(2, 8)
        # fewer queries than the arrays hold: nothing behind Q, or Q * K, is written
        assert look.run(2, 8, Q=7) == 0 and look.holds(want, Q=7)


def test_errors_return_before_any_launch():
    rng = np.random.default_rng(15)
    V = 8
    entries = [word(rng, V, int(rng.integers(1, 9))) for _ in range(200)]
    queries = [mutate(rng, entries[i], V, 1) for i in range(20)]
    look = Look(entries, queries, V)
    cf = look.class_first
    assert look.n_ws % 8 == 0 and look.n_ws == look.lib.kl_lexicon_neighbours_workspace_bytes(1, 1)
    down, short, late, none = cf.copy(), cf.copy(), cf.copy(), cf * 0
    down[5] = down[4] - 1 if down[4] > 0 else down[6] + 1          # decreases
    short[65] += 1                                                   # one entry more than n_chars holds ids for
    late[1] = 1                                                      # class_first[1] != 0
    cases = [dict(table=down), dict(table=short), dict(table=late), dict(table=none),
             dict(n_chars=len(look.layout[0]) + 1), dict(V=0), dict(V=4097), dict(Q=0), dict(Q=2 ** 31),
             dict(n_q=2 ** 40 + 1), dict(n_chars=2 ** 40 + 1)]
    cases += [{name: None} for name in look.NAMES + ("class_first", "ws")]
    cases += [dict(shift={name: 2}) for name in ("chars", "order", "q_pool", "exact", "found", "cand", "dist")]
    cases += [dict(shift={name: 4}) for name in ("q_off", "class_first", "ws")]
    for case in cases:
        assert look.run(2, 8, **case) == KL_ERR_ARG, case
        assert look.untouched(), case
    for max_dist, K in ((-1, 8), (9, 8), (2, 0), (2, 17)):
        assert look.run(max_dist, K, room=16) == KL_ERR_ARG and look.untouched(), (max_dist, K)
    assert look.run(2, 8, ws_bytes=look.n_ws - 1) == KL_ERR_WORKSPACE and look.untouched()
    look.is_statement(2, 8)
    look.is_statement(8, 16)


# ---------------------------------------------------------------------------------------------- engine and Rater
def test_engine_wrapper_and_rater_lexicon_neighbours():
    from ocrd_keraslm_amd.lib import hipabi
    from tests.test_rater_golden import hip_factory
    torch, dev = device()
    cfg, w, lm = make_model(2, 64, 20, 1)
    rng = np.random.default_rng(16)
    V = 20
    entries = [word(rng, V, int(rng.integers(1, 9))) for _ in range(500)]
    queries = [mutate(rng, entries[int(rng.integers(0, 500))], V, int(rng.integers(0, 3))) for _ in range(50)] + [[], [3] * 65]
    chars, order, class_first = ratebulk.lexicon_layout_host(*pooled(entries))
    q_pool, q_off = pooled(queries)
    want = ratebulk.lexicon_neighbours_host(q_pool, q_off, chars, order, class_first, V, 2, 5)
    got = lm.lexicon_neighbours(up(chars), up(order), class_first, V, up(q_pool), up(q_off), 2, 5)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got) and [tuple(t.shape) for t in got] == [(52,), (52,), (52, 5), (52, 5)]
    for g, r in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), r)
    for wrong in (dict(chars=up(chars).long()), dict(q_off=up(q_off).int()), dict(order=up(order)[::2]), dict(q_pool=torch.from_numpy(q_pool)),
                  dict(class_first=class_first[:-1]), dict(K=17), dict(max_dist=9), dict(V=4097)):
        a = dict(dict(chars=up(chars), order=up(order), class_first=class_first, V=V, q_pool=up(q_pool), q_off=up(q_off), max_dist=2,
                      K=5), **wrong)
        with pytest.raises(hipabi.KlError):
            lm.lexicon_neighbours(a["chars"], a["order"], a["class_first"], a["V"], a["q_pool"], a["q_off"], a["max_dist"], a["K"])
    # the Rater: normalised, unique, spread back over the duplicates; the device copy of the lexicon is made once
    hip = small_rater(hip_factory)
    assert hasattr(hip.model, "lexicon_neighbours")
    lex = hip.lexicon(lexicon_words(rng, 400))
    words = lexicon_words(rng, 60) + [lex.words[9], "a?c", "", "ab" * 40]
    words += words[:9]
    near = hip.lexicon_neighbours(words, lex, max_dist=2, per_word=6)
    held = lex.on_device(hip.model)
    pool, off = pooled([[hip.mapping[0].get(c, 0) for c in w] for w in words])
    want = ratebulk.lexicon_neighbours_host(pool, off, lex.chars, lex.order, lex.class_first, hip.voc_size, 2, 6)
    for g, r in zip((near.exact, near.found, near.index, near.dist), want):
        assert g.dtype == np.int32 and np.array_equal(g, r)
    assert near.exact[60] == 9 and near.found.max() > 6
    again = hip.lexicon_neighbours(words[:5], lex, max_dist=1, per_word=2)
    assert all(a is b for a, b in zip(held, lex.on_device(hip.model))) and np.array_equal(again.exact, near.exact[:5])
    none = hip.lexicon_neighbours([], lex)
    assert len(none) == 0 and none.index.shape == (0, 8)


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_rater_correct_words_is_the_composed_call(precision):
    """a dozen short texts, a lexicon of a few hundred entries: the same words, the same edits, and every field of the result
    identical to `rescore` called by hand on these edits -- it is the same code path"""
    from tests.test_rater_golden import hip_factory
    texts, contexts = contract_texts()
    rng = np.random.default_rng(17)
    texts = list(texts) + [random_text(rng, 30) for _ in range(3)]
    contexts = list(contexts) + [[175]] * 3
    hip = small_rater(hip_factory)
    rule = dict(k=2, streams=4, max_prob=1.0, min_rank=0, min_suspects=0)
    everything, _ = hip.suspect_words(texts, contexts, precision=precision, **rule)
    in_text = sorted(set(w for one, t in zip(everything, texts) for w in one.strings(t) if len(w) > 1))
    lex = hip.lexicon(in_text[::3] + lexicon_words(rng, 300))
    rescoring = dict(streams=4, left=12, ahead=3, min_gain=0.5)
    n_edits = {}
    for known in (False, True):
        found, rescored, bits = hip.correct_words(texts, lex, contexts, max_dist=1, per_word=3, known=known, precision=precision,
                                                  **dict(rule, **rescoring))
        ref_found, edits, ref_rescored, ref_bits = composed(hip, texts, contexts, lex, 1, 3, known, dict(rule, precision=precision),
                                                            dict(rescoring, precision=precision))
        assert np.array_equal(bits, ref_bits)
        for one, ref in zip(found, ref_found):
            assert one.spans() == ref.spans() and np.array_equal(one.bits, ref.bits)
        same_rescored(rescored, ref_rescored)
        assert sum(len(one) for one in rescored) == len(edits) > 0 and sum(int((one.best >= 0).sum()) for one in rescored) > 0
        n_edits[known] = len(edits)
        assert bool([1 for i, a, b, _ in edits if texts[i][a:b] in lex.words]) == known
    assert n_edits[True] > n_edits[False]
    assert hip.model.states.shape[0] == 1 and not hip.model.states.cpu().numpy().any()


def test_cli_lexicon_on_the_device(tmp_path):
    from ocrd_keraslm_amd.scripts import run
    from tests.test_rater_golden import hip_factory
    model = str(tmp_path / "model.h5")
    small_rater(hip_factory).save(model)
    rng = np.random.default_rng(18)
    files, texts = [], []
    for i, size in enumerate((90, 70)):
        name = tmp_path / ("auth_title%d_%d.txt" % (i, 1700 + 40 * i))
        texts.append(random_text(rng, size))
        name.write_text(texts[-1])
        files.append(str(name))
    entries = lexicon_words(rng, 300)
    listing = tmp_path / "words.tsv"
    listing.write_text("".join("%s\t%d\n" % (w, i) for i, w in enumerate(entries)))
    res = CliRunner().invoke(run.cli, ["lexicon", "-m", model, "--lexicon", str(listing), "--apply", "-s", "4", "-k", "2", "--max-prob",
                                       "1", "--min-rank", "0", "--min-suspects", "0", "--max-dist", "1", "--per-word", "4", "--left",
                                       "10", "--ahead", "2", "--min-gain", "0.25"] + files)
    assert res.exit_code == 0, res.output + repr(res.exception)
    lines = [json.loads(l) for l in res.output.strip().split("\n")]
    assert [l["file"] for l in lines] == files
    ref = run._load(model)
    assert hasattr(ref.model, "lexicon_neighbours")
    _, found, _ = ref.correct_words(texts, ref.lexicon(entries), [[170], [174]], max_dist=1, per_word=4, k=2, max_prob=1.0, min_rank=0,
                                    min_suspects=0, left=10, ahead=2, min_gain=0.25, streams=4)
    assert sum(int((f.best >= 0).sum()) for f in found) > 0
    for line, text, one in zip(lines, texts, found):
        assert type(one) is ratebatch.Rescored and line["chars"] == len(text) and line["corrected"] == one.apply(text)
        assert line["rescored"] == [[int(a), int(b), text[int(a):int(b)], new, float(g)]
                                    for a, b, new, g in zip(one.starts, one.ends, one.proposals(), one.gain)]
