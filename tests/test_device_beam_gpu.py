"""The device beam of `Rater.generate` on the GPU (-m gpu), all through the C ABI:
  * kl_beam_expand against genbeam.expand_host on synthetic device arrays whose candidate costs are built at least 1e-4
    (relative) apart -- or bitwise equal --, so that the order cannot hinge on the few ulps by which logf and numpy's float32
    log may differ: parents, ids, slots and the live count exactly, costs within 2e-6 relative (about 16 ulp: two logs good
    to a few ulp each and one float32 addition);
  * `Rater.generate` on the HIP engine, device beam against the host path: same strings, costs within 1e-3 (the project's
    bar on probabilities; the host path's step uses another softmax launch), twice bitwise the same;
  * the refusals of kl_beam_expand, with nothing launched."""
import ctypes as C

import numpy as np
import pytest

from oracle import lstm_oracle as O
from ocrd_keraslm_amd.lib import Rater, genbeam
from tests.oracle_engine import OracleLM

pytestmark = pytest.mark.gpu

FLOOR = np.float32(0.004)
BELOW = np.nextafter(FLOOR, np.float32(0))
ZERO_SLOT = 5
REL_APART = 1e-4


def build_case(V, rows, fan, live, seed):
    """probs [rows][V], cum_in [rows], slot_new [rows]: every candidate's running cost sits on its own point of a geometric
    lattice (ratio 1 + 3e-4) -- p = exp(-(point - cum_in[row])) --, so distinct costs are >= 1e-4 relative apart.  Built in:
    dead rows between live ones, peaked rows (one to three candidates) and full ones, id 0 and id 5 (which the mask removes) with large
    probabilities, 0.004f and the float32 below it, and bitwise-equal duplicate rows with equal cum_in (exact ties)."""
    rng = np.random.default_rng(seed)
    ratio = 1.0 + 3e-4
    if live == "all":
        live_rows = np.arange(rows)
    elif live == 1:
        live_rows = np.array([2])
    else:      # rows 1 and 2 are dead, and more in between
        live_rows = np.array([0] + sorted(rng.choice(np.arange(3, rows - 1), size=live - 2, replace=False).tolist()) + [rows - 1])
    probs = (rng.uniform(1e-5, 3e-3, (rows, V))).astype(np.float32)      # below the floor everywhere (dead rows keep this)
    cum = np.full(rows, np.inf, dtype=np.float32)
    used = set()
    floor_cost = float(-np.log(np.float64(FLOOR)))

    def point(m):
        return 0.05 * ratio ** m

    def index(x):
        return np.log(x / 0.05) / np.log(ratio)

    for n, r in enumerate(live_rows):
        ids = rng.permutation(np.arange(1, V))
        ids = ids[ids != 5]
        k = int(rng.integers(1, 4)) if n % 3 == 1 else int(rng.integers(max(1, fan - 3), fan + 1))
        special = n % 4 == 0      # exactly the floor (kept) and the float32 below it (dropped), both among the `fan` largest
        if special:
            k = min(k, fan - 4)
        while True:               # cum_in on the lattice, 0.09 .. 3.3; a special row's: one that keeps the floor's cost clear of all others
            base = np.float32(point(int(rng.integers(2000, 14000))))
            near = int(round(index(float(base) + floor_cost)))
            if not special or not used & set(range(near - 2, near + 3)):
                break
        cum[r] = base
        if special:
            probs[r, ids[-1]], probs[r, ids[-2]] = FLOOR, BELOW
            used.update(range(near - 2, near + 3))
        lo, hi = int(np.ceil(index(float(base) + 0.06))), int(np.floor(index(float(base) + 5.3)))
        # (id 5 is a candidate without the mask: its cost is on the lattice too, p = 0.3 .. 0.9)
        for v, m_lo, m_hi in [(ids[j], lo, hi) for j in range(k)] + ([(5, lo + 200, int(index(float(base) + 1.2)))] if n % 5 == 0 else []):
            while True:
                m = int(rng.integers(m_lo, m_hi))
                if m not in used:
                    break
            used.add(m)
            probs[r, v] = np.float32(np.exp(-(point(m) - float(base))))
        if n % 2 == 0:
            probs[r, 0] = np.float32(rng.uniform(0.3, 0.9))          # id 0 among the `fan` largest: it holds a place
    # duplicates: a live row repeated bitwise (with its cum_in) in the next live row
    for a, b in zip(live_rows[0::6], live_rows[1::6]):
        probs[b], cum[b] = probs[a], cum[a]
    slot_new = (1000 + rng.permutation(rows)).astype(np.int32)
    return probs, cum, slot_new


@pytest.fixture(scope="module")
def beam_lib():
    import torch
    from ocrd_keraslm_amd.lib import hipabi
    assert torch.cuda.is_available()
    lib = hipabi.load()
    handles = {}

    def handle(V):
        if V not in handles:
            cfg = hipabi.KlConfig(1, 64, V, 1, 200, 10)
            handles[V] = lib.kl_create(C.byref(cfg))
            assert handles[V]
        return handles[V]

    yield lib, handle
    torch.cuda.synchronize()
    for h in handles.values():
        lib.kl_destroy(h)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def run_expand(lib, h, probs, cum, slot_new, valid, rows, fan, ws_bytes=None, null_probs=False):
    """kl_beam_expand on the current stream; returns its code and the ten output arrays (numpy), prefilled with a sentinel"""
    import torch
    dev = torch.device("cuda:0")
    p_d = torch.from_numpy(probs).to(dev)
    c_d = torch.from_numpy(cum).to(dev)
    s_d = torch.from_numpy(slot_new).to(dev)
    v_d = torch.from_numpy(valid).to(dev) if valid is not None else None
    n_out = max(rows, 1)
    ints = [torch.full((n_out,), -77, dtype=torch.int32, device=dev) for _ in range(4)]      # idx_next, slot_in_next, parent, idx_log
    flts = [torch.full((n_out,), -77.0, dtype=torch.float32, device=dev) for _ in range(2)]    # cum_next, cum_log
    n_live = torch.full((1,), -77, dtype=torch.int32, device=dev)
    need = int(lib.kl_beam_workspace_bytes(h, rows, fan))
    ws = torch.zeros(max(need, 1 << 16), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    code = lib.kl_beam_expand(h, rows, fan, float(FLOOR), _ptr(None if null_probs else p_d), _ptr(v_d), _ptr(c_d), _ptr(s_d),
                              ZERO_SLOT, _ptr(ints[0]), _ptr(ints[1]), _ptr(flts[0]), _ptr(ints[2]), _ptr(ints[3]), _ptr(flts[1]),
                              _ptr(n_live), _ptr(ws), need if ws_bytes is None else ws_bytes, stream)
    torch.cuda.synchronize()
    return code, need, [t.cpu().numpy() for t in ints], [t.cpu().numpy() for t in flts], int(n_live.item())


@pytest.mark.parametrize("live", [1, 7, "all"])
@pytest.mark.parametrize("rows,fan", [(16, 10), (256, 10), (256, 16)])
@pytest.mark.parametrize("V", [40, 64, 300])
def test_beam_expand_matches_expand_host(beam_lib, V, rows, fan, live):
    lib, handle = beam_lib
    probs, cum, slot_new = build_case(V, rows, fan, live, seed=V * 1000 + rows + fan)
    n_live_rows = int((cum < np.inf).sum())
    assert n_live_rows == (rows if live == "all" else live)
    mask = np.ones(V, dtype=np.uint8)
    mask[[0, 5]] = 0
    for valid in (None, mask):
        idx, slot_in, cum_next, parent, n_live = genbeam.expand_host(probs, cum, valid, rows, fan, FLOOR, slot_new, ZERO_SLOT)
        # the pre-condition, on the numpy result itself: distinct candidate costs (ALL candidates, not only the survivors) are
        # at least 1e-4 relative apart, so a few ulp cannot change the order; equal ones are the built ties
        c_row, c_id, c_cum, _seq = genbeam.candidates_host(probs, cum, valid, rows, fan, FLOOR)
        all_cum = np.sort(c_cum.astype(np.float64))
        gaps = np.diff(all_cum)
        assert ((gaps == 0) | (gaps >= REL_APART * all_cum[1:])).all(), (gaps[gaps > 0].min(), V, rows, fan, live)
        n_cand = len(all_cum)
        # what the case is there for
        if live == "all":
            assert n_cand > rows and n_live == rows and (gaps == 0).sum() >= 3          # truncation, exact ties
        if live == 7:
            assert (gaps == 0).any() and cum[1] == np.inf and cum[2] == np.inf          # ties; dead rows between live ones
            assert (n_cand > rows) == (rows == 16)                                      # more candidates than rows, or fewer
        if live == 1:
            assert 0 < n_live < rows and not (gaps == 0).any()
        alive = cum < np.inf
        assert (probs[alive][:, 0] >= np.sort(probs[alive], axis=1)[:, -fan]).any()     # id 0 among the `fan` largest
        cand_p = probs[c_row, c_id]
        assert (cand_p == FLOOR).any() and (probs[alive] == BELOW).any() and (cand_p >= FLOOR).all()      # 0.004f kept, the value below dropped
        assert (c_id != 0).all() and (valid is None or (c_id != 5).all())
        code, _need, ints, flts, got_live = run_expand(lib, handle(V), probs, cum, slot_new, valid, rows, fan)
        assert code == 0
        assert got_live == n_live
        assert np.array_equal(ints[2], parent)
        assert np.array_equal(ints[0], idx) and np.array_equal(ints[3], idx)
        assert np.array_equal(ints[1], slot_in)
        assert np.array_equal(flts[0], flts[1])                                          # (bitwise: the same value stored twice)
        assert np.isinf(flts[0][n_live:]).all() and (flts[0][n_live:] > 0).all()
        assert (ints[2][n_live:] == -1).all() and (ints[1][n_live:] == ZERO_SLOT).all() and (ints[0][n_live:] == 0).all()
        rel = np.abs(flts[0][:n_live].astype(np.float64) - cum_next[:n_live]) / cum_next[:n_live]
        print("V %d rows %d fan %d live %s mask %s: %d candidates, %d survivors, max rel cum error %.3g"
              % (V, rows, fan, live, valid is not None, n_cand, n_live, rel.max() if n_live else 0.0))
        assert (rel <= 2e-6).all()
        # the built ties stay ties on the device: equal reference costs, equal device costs
        same = np.flatnonzero(np.diff(cum_next[:n_live]) == 0)
        assert (flts[0][same] == flts[0][same + 1]).all()


def test_beam_expand_refusals_launch_nothing(beam_lib):
    from ocrd_keraslm_amd.lib import hipabi
    lib, handle = beam_lib
    V = 40
    probs, cum, slot_new = build_case(V, 256, 10, 7, seed=3)
    KL_ERR_WORKSPACE, KL_ERR_ARG = 4, 5
    assert lib.kl_error_string(KL_ERR_WORKSPACE).decode().startswith("workspace")
    assert lib.kl_error_string(KL_ERR_ARG).decode().startswith("null or invalid")
    need = int(lib.kl_beam_workspace_bytes(handle(V), 256, 10))
    assert need >= 256 * 10 * 12
    assert lib.kl_beam_workspace_bytes(handle(V), 0, 10) == lib.kl_beam_workspace_bytes(handle(V), 257, 10) == 0
    assert lib.kl_beam_workspace_bytes(handle(V), 256, 17) == lib.kl_beam_workspace_bytes(handle(V), 256, 0) == 0
    for kw, want in ((dict(rows=0, fan=10), KL_ERR_ARG), (dict(rows=257, fan=10), KL_ERR_ARG), (dict(rows=256, fan=17), KL_ERR_ARG),
                     (dict(rows=256, fan=10, null_probs=True), KL_ERR_ARG), (dict(rows=256, fan=10, ws_bytes=need - 1), KL_ERR_WORKSPACE)):
        big = max(kw["rows"], 256)
        p = np.resize(probs, (big, V))
        code, _need, ints, flts, got_live = run_expand(lib, handle(V), p, np.resize(cum, big), np.resize(slot_new, big), None, **kw)
        assert code == want, (kw, code)
        # nothing was launched: every output still holds its sentinel
        assert got_live == -77 and all((a == -77).all() for a in ints) and all((a == -77.0).all() for a in flts), kw
    with pytest.raises(hipabi.KlError):
        hipabi.check(KL_ERR_ARG, "kl_beam_expand")


# ---------------------------------------------------------------------- Rater.generate on the HIP engine
class TopsOracle(OracleLM):
    """the f64 CPU double, keeping the median top probability of every step"""

    def step_slots(self, *args):
        p = super().step_slots(*args)
        self.tops = getattr(self, "tops", []) + [float(np.median(p.max(axis=1)))]
        return p


def hip_factory(*args):
    from ocrd_keraslm_amd.lib.engine import HipLM
    return HipLM(*args)


def generate_rater(factory, depth, width, seed, emb_std):
    chars = [chr(c) for c in range(0x41, 0x41 + 60)]
    r = Rater(engine_factory=factory)
    r.width, r.depth, r.length = width, depth, 8
    r.stateful, r.incremental = False, True
    r.mapping = ({c: i + 1 for i, c in enumerate(chars)}, {i + 1: c for i, c in enumerate(chars)})
    r.voc_size = len(chars) + 1
    r.configure()
    cfg = O.ModelConfig(depth, width, r.voc_size, 1)
    r.model.set_weights(O.init_weights(cfg, seed=seed, emb_std=emb_std, dtype=np.float64), 3)
    r.status = 2
    return r


# (seed, emb_std) chosen on the CPU double: the four cheapest final costs 1e-2 apart (0.41 / 0.22 / 0.19 and 0.20 / 0.20 / 0.17),
# median top probability 0.45 and 0.61
@pytest.mark.parametrize("depth,width,seed,emb_std", [(2, 128, 1, 2.0), (1, 64, 1, 2.0)])
def test_generate_device_beam_on_the_hip_engine_equals_host_path(depth, width, seed, emb_std):
    prefix, length, ctx = "HELLO", 12, [17]
    cpu = generate_rater(TopsOracle, depth, width, seed, emb_std)
    cpu_strings = cpu.generate(prefix, length, ctx, 4)
    assert np.median(cpu.model.tops[len(prefix) - 1:]) > 0.3                             # a peaked model
    assert (np.diff(cpu.generate_costs) >= 1e-2).all(), cpu.generate_costs
    r = generate_rater(hip_factory, depth, width, seed, emb_std)
    assert hasattr(r.model, "beam_expand") and r.device_beam is False
    host = r.generate(prefix, length, ctx, 4, device_beam=False)
    host_costs = list(r.generate_costs)
    assert len(host_costs) == 4 and (np.diff(host_costs) >= 1e-3).all(), host_costs      # the pre-condition, on the host path's own result
    assert host == cpu_strings
    pool = r._state_pool()
    free = sorted(pool.free)
    got = r.generate(prefix, length, ctx, 3, device_beam=True)
    costs = list(r.generate_costs)
    print("depth %d width %d: %r, costs host %r device %r" % (depth, width, got, host_costs[:3], costs))
    assert got == host[:3]
    assert all(len(s) == length + 1 and s[0] == prefix[-1] for s in got)
    assert len(costs) == 3 and np.abs(np.array(costs) - np.array(host_costs[:3])).max() <= 1e-3
    assert sorted(pool.free) == free
    again = r.generate(prefix, length, ctx, 3, device_beam=True)
    assert again == got and r.generate_costs == costs                                    # bitwise the same
    # a one-character prefix (no warm-up) and length 0
    assert r.generate("Q", 4, ctx, 2, device_beam=True) == r.generate("Q", 4, ctx, 2, device_beam=False)
    assert r.generate(prefix, 0, ctx, 2, device_beam=True) == ["O"]
