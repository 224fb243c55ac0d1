"""What the four lexicon look-ups share in front of their walks, on the GPU (run with -m gpu on an MI355X): a query outside the
pool -- an offset below 0, an end beyond n_q --, of no ids or of more than 64 is "none" in kl_lexicon_neighbours,
kl_lexicon_channel, kl_lexicon_splits and kl_lexicon_chains alike: nothing of it is read, its rows are the constants, and the
queries around it are looked up as if they stood alone.

No host statement covers this (the four `*_host` functions raise on such offsets), so a valid row is held to the statement run
on that query alone and a none row to its constants, bit for bit, with the guard bands of the harness classes behind every
output.  The pool is a view 16 elements into a larger buffer, and what lies outside the pool -- in front of it and behind n_q --
spells words that the lexicon holds: a look-up that read there would not fault, it would find them."""
import numpy as np
import pytest

from ocrd_keraslm_amd.lib import ratebulk
from tests.test_lexicon_chains_gpu import Chain
from tests.test_lexicon_channel_gpu import Chan
from tests.test_lexicon_gpu import Look, word
from tests.test_lexicon_splits_gpu import Cut
from tests.test_rate_window_gpu import ptr
from tests.test_rate_words_gpu import up

pytestmark = pytest.mark.gpu

V, K, P = 8, 4, 3
FRONT, POOL = 16, 80

# per entry point: the harness, its outputs, what `run` takes in front, and the statement for (pool, off) on the layout of h
LOOKUPS = {
    "neighbours": (Look, ("exact", "found", "cand", "dist"), (2, K),
                   lambda h, pool, off: ratebulk.lexicon_neighbours_host(pool, off, *h.layout, h.V, 2, K)),
    "channel": (Chan, ("exact", "found", "cand", "cost"), (1, 2, K),
                lambda h, pool, off: ratebulk.lexicon_channel_host(pool, off, *h.layout, h.V, h.rules[0], h.rules[1], 1, 2, K)),
    "splits": (Cut, ("found", "split", "left", "right", "dist"), (2, 1, K),
               lambda h, pool, off: ratebulk.lexicon_splits_host(pool, off, *h.layout, h.V, 2, 1, K)),
    "chains": (Chain, ("found", "worst", "entry", "start", "link"), ([], P, 1),
               lambda h, pool, off: ratebulk.lexicon_chains_host(pool, off, *h.layout, h.V, [], P, 1)),
}


def alone(statement, h, ids):
    """the statement's rows for one query of these ids"""
    return statement(h, np.asarray(ids, dtype=np.int32), np.asarray([0, len(ids)], dtype=np.int64))


def constant(outputs, o):
    return 0 if outputs[o] == "found" else -1


def is_none(rows, outputs):
    return all((a[0] == constant(outputs, o)).all() for o, a in enumerate(rows))


@pytest.mark.parametrize("name", sorted(LOOKUPS))
def test_queries_outside_the_pool_empty_or_too_long_are_none_and_the_others_stand_alone(name):
    harness, outputs, front, statement = LOOKUPS[name]
    rng = np.random.default_rng(40)
    five, nine = word(rng, V, 5), word(rng, V, 9)
    entries = [word(rng, V, int(rng.integers(1, 9))) for _ in range(40)]
    buffer = rng.integers(0, V, FRONT + POOL + 16).astype(np.int32)
    buffer[FRONT - 2:FRONT + 3] = five          # pool[-2:3]
    buffer[FRONT + 71:FRONT + 80] = nine        # pool[71:80]
    buffer_d = up(buffer)
    pool = buffer[FRONT:FRONT + POOL]
    # every word the calls look up or must not look up is an entry, two entries run together and a chain of two
    for w in (five, nine[:8], nine, pool[0:3].tolist(), pool[3:6].tolist(), pool[68:71].tolist()):
        entries += [w[:64], w[:len(w) // 2], w[len(w) // 2:]]
    calls = [([0, 3, 3, 68, 71, 80], 75, (0, 3), nine),      # 1: no ids, 2: 65 ids, 4: ends beyond n_q
             ([-2, 3, 6], POOL, (1,), five)]                  # 0: begins in front of the pool
    for off, n_q, valid, outside in calls:
        Q = len(off) - 1
        h = harness(entries, [[0]] * Q, V)
        assert not is_none(alone(statement, h, outside), outputs)      # what lies outside the pool would be found if it were read
        want = None
        for q in valid:
            rows = alone(statement, h, pool[off[q]:off[q + 1]])
            if want is None:
                want = [np.full((Q,) + a.shape[1:], constant(outputs, o), dtype=np.int32) for o, a in enumerate(rows)]
            for w, a in zip(want, rows):
                w[q] = a[0]
        assert not any(is_none([w[q:] for w in want], outputs) for q in valid)
        off_d = up(np.asarray(off, dtype=np.int64))
        assert h.run(*front, q_pool=ptr(buffer_d[FRONT:]), q_off=ptr(off_d), n_q=n_q) == 0
        assert h.holds(want), (name, off)
