"""Shared pieces of the edge-walk tests (tests/test_edge_walk.py, tests/test_edge_walk_gpu.py) -- TEST INFRASTRUCTURE:
random lattices from fixed seeds, a logger that keeps its messages, a CPU engine with `walk_host` answered by chained
oracle steps, and the comparison of two `rate_best` results."""
import numpy as np

from oracle import lstm_oracle as O
from tests.oracle_engine import OracleLM
from tests.test_rater_golden import SEAM, lattice

CHARS = SEAM["model"]["chars"]
UNMAPPED = "#%"      # not in the golden model's character set


def random_segments(seed, n_edges=30, max_alts=6, max_len=10, unmapped=True, empty=True):
    """[[(text, conf)]] per edge: 1 .. max_alts alternatives of 1 .. max_len characters; some characters unmapped; the LAST
    edge also carries an empty alternative (the decoder -- ours as the reference's -- reads the last character of a
    hypothesis' text when it continues it, so an empty alternative can only stand where nothing follows; it costs nothing --
    the confidence term is paid per character -- and so heads the final beam: `run_pages(finish=False)` for such lattices,
    the score of a committed segment divides by its length)."""
    rng = np.random.default_rng(seed)
    letters = [c for c in CHARS if c != "\n"]
    segs = []
    for e in range(n_edges):
        last = e == n_edges - 1
        n_alt = int(rng.integers(1, max_alts + 1 - (2 if last and empty else 0)))
        alts = []
        for _ in range(n_alt):
            text = "".join(letters[int(k)] for k in rng.integers(0, len(letters), size=int(rng.integers(1, max_len + 1))))
            if unmapped and rng.random() < 0.15:
                at = int(rng.integers(0, len(text)))
                text = text[:at] + UNMAPPED[int(rng.integers(0, len(UNMAPPED)))] + text[at + 1:]
            alts.append((text, float(rng.uniform(0.05, 1.0))))
        if last and empty:
            alts.append(("e", 0.99))
            alts.append(("", 0.5))
        segs.append(alts)
    return segs


class KeepLogger(object):
    """stands in for logging.Logger: keeps the formatted error messages in order"""

    def __init__(self):
        self.errors = []

    def error(self, msg, *args):
        self.errors.append(msg % args)

    def debug(self, *_args):
        pass

    info = warning = critical = debug


class WalkOracle(OracleLM):
    """OracleLM with `walk_host`: the rows' chained oracle steps (f64), every call recorded"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.walk_calls = []       # (rows, lens) per call
        self.steps_taken = 0       # step_slots calls (an edge walk makes none)

    def step_slots(self, *args, **kwargs):
        self.steps_taken += 1
        return super().step_slots(*args, **kwargs)

    def walk_host(self, lens, idx, target, ctx, slot_in, slot_step, head_k=0, timeout=20.0):
        lens = [int(k) for k in lens]
        tprob, last = chained_reference(self.cfg, self.w, self.pool, lens, idx, target, ctx, slot_in, slot_step)
        self.walk_calls.append((len(lens), lens))
        heads = self.pool[last, :head_k].copy() if head_k else None
        return tprob, heads


def chained_reference(cfg, w, pool, lens, idx, target, ctx, slot_in, slot_step):
    """len[i] chained oracle steps per row on the numpy pool [slots][2L][W] (written in place); returns (tprob ragged f64,
    final slot per row).  The reference of the walk's C ABI: oracle steps, not kl_step_batch."""
    n = len(lens)
    idx, target, slot_step = np.asarray(idx).reshape(-1), np.asarray(target).reshape(-1), np.asarray(slot_step).reshape(-1)
    ctx = np.asarray(ctx).astype(np.int64).reshape(n, cfg.n_ctx)
    slot_in = np.asarray(slot_in).reshape(-1)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    assert len(set(slot_step.tolist())) == len(slot_step), "slot_step entries must be distinct"
    assert not set(slot_step.tolist()) & set(slot_in.tolist()), "slot_step must not name a slot_in"
    tprob = np.zeros(int(np.sum(lens)), dtype=np.float64)
    depth2 = pool.shape[1]
    for t in range(max(lens)):
        rows = np.array([i for i in range(n) if lens[i] > t])
        at = off[rows] + t
        src = slot_in[rows] if t == 0 else slot_step[at - 1]
        states = [pool[src, k] for k in range(depth2)]
        probs, new = O.step_batch(cfg, w, idx[at].astype(np.int64), ctx[rows], states)
        for k in range(depth2):
            pool[slot_step[at], k] = new[k]
        tprob[at] = probs[np.arange(len(rows)), target[at]]
    return tprob, slot_step[off + np.asarray(lens) - 1]


def run_pages(rater, pages, lm_weight=0.5, beam_width=10, dist=0, edge_walk=None, context=(17,), finish=True):
    """rate_best over consecutive pages with carried traceback, then (finish) the final path; what is comparable of it"""
    traceback = None
    out = []
    kw = {} if edge_walk is None else {"edge_walk": edge_walk}
    for segs in pages:
        g, s, e = lattice(segs)
        path, entropy, traceback = rater.rate_best(g, s, e, start_traceback=traceback, context=list(context), lm_weight=lm_weight,
                                                   beam_width=beam_width, beam_clustering_dist=dist, **kw)
        out.append(summary(path, entropy, traceback))
    if finish:
        path, entropy, traceback = rater.next_path(traceback[0], ([], traceback[1]))
        out.append(summary(path, entropy, traceback))
    return out


def summary(path, entropy, traceback):
    return {"path": [(el.id, alt.Unicode, alt.index) for el, alt, _ in path],
            "scores": [float(s) for _, _, s in path],
            "entropy": float(entropy),
            "beam": [((n.extras[0].id, n.extras[1].index) if n.extras else None) for n in traceback[0]],
            # every surviving hypothesis as the alternatives it went through since the last committed node
            "hyps": [[(m.extras[0].id, m.extras[1].index) for m in n.to_sequence() if m.extras] for n in traceback[0]],
            "costs": [float(n.cum_cost) for n in traceback[0]]}
