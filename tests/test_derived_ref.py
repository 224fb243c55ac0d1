"""The derived-operand comparator (tests/derived_ref.py) without a GPU: every array built from its definition for a small
model (depth 2, width 64, 5 characters padded to 32 table rows, two context variables of 6 values x 3 dimensions, split
precision, every group current), then one mistake at a time of the kinds `kl_prepare` and its lazy companions can make --
each must fail, on exactly the array it belongs to, at the place it was made.  Arrays DERIVED from a wrong one are rebuilt
from it, as the device would: the comparator holds them to what was read back, so the mistake stays where it was made.
This is the evidence that tests/test_derived_gpu.py's passing means what it says."""
import numpy as np
import pytest

from tests import derived_ref as D

SH = D.Shape(2, 64, 5, 2, ctx_vocab=6, ctx_dim=3)
W, V, Vp, R = SH.width, SH.voc_size, SH.Vp, SH.ctx_vocab
PREC = D.PREC_SPLIT


@pytest.fixture(scope="module")
def clean():
    params = D.random_params(SH, 11)
    return params, D.build_exact(SH, params, PREC)


def _copy(g):
    return {k: v.copy() for k, v in g.items()}


def _downstream(g, params, ekp=None):
    """what the device derives from EK / CtxK / EKp as stored (ekp: a wrong EKp to go on from)"""
    w = D.weights(SH, params)
    g["EKp"] = D.ekp_from(g["EK"], w["b0"], W) if ekp is None else ekp
    for n in range(SH.n_ctx):
        g["CtxKp[%d]" % n] = D.interleave_cols(g["CtxK[%d]" % n], W)
    g["comb"] = D.comb_from(g["EKp"], g["CtxKp[0]"])
    return g


def _fails(params, g, current=D.ALL_GROUPS, precision=PREC):
    with pytest.raises(D.DerivedMismatch) as e:
        D.compare(SH, params, precision, current, g, where="injected")
    return e.value


def test_clean_set_passes(clean):
    params, g = clean
    out = D.compare(SH, params, PREC, D.ALL_GROUPS, g)
    assert set(out["checked"]) == set(g), set(g) ^ set(out["checked"])      # nothing built is left unchecked
    assert out["stats"]["EK_array"] < 0.01 and out["stats"]["EK_row"] < 0.01 and out["stats"]["CtxK"] < 1.0, out["stats"]
    # ... and in bf16 precision, where EK is held to the product of the rounded operands and one plane is written
    gb = D.build_exact(SH, params, D.PREC_BF16)
    out = D.compare(SH, params, D.PREC_BF16, D.ALL_GROUPS & ~D.LO, gb)
    assert "UT_lo[0]" not in out["checked"] and "UF[1]" in out["checked"]
    # the bf16 EK is NOT the split EK: the two references are told apart by their bounds
    assert "EK" in _fails(params, dict(g, EK=gb["EK"])).arrays


def test_definitions_are_permutations(clean):
    """the layout helpers against index-by-index loops (the statements of the module's docstring)"""
    _, g = clean
    kt, ktp = g["KT_hi[1]"], g["KTp[1]"]
    perm, cat = g["WTperm[1]"], g["WTcat[1]"]
    for u in (0, 1, 31, 32, 63):
        for gate in range(4):
            assert np.array_equal(ktp[u * 4 + gate], kt[gate * W + u])
            assert np.array_equal(perm[(u // 32) * 128 + gate * 32 + u % 32], cat[gate * W + u])
            assert g["EKp"][3, u * 4 + gate] == np.float32(g["EK"][3, gate * W + u] + D.weights(SH, clean[0])["b0"][0, gate * W + u])
    uf = g["UF[0]"]
    for rt, kb, lane in ((0, 0, 0), (3, 1, 17), (15, 1, 63), (7, 0, 48)):
        c, q = lane % 16, lane // 16
        assert np.array_equal(uf[rt, kb, 0, lane], g["UT_hi[0]"][rt * 16 + c, kb * 32 + 8 * q:kb * 32 + 8 * q + 8])
        assert np.array_equal(uf[rt, kb, 1, lane], g["UT_lo[0]"][rt * 16 + c, kb * 32 + 8 * q:kb * 32 + 8 * q + 8])
    assert np.array_equal(g["comb"][2 * R + 4], D.bf16_bits(g["EKp"][2] + g["CtxKp[0]"][4]))
    assert cat.shape == (4 * W, 6 * W) and np.array_equal(cat[:, :W], g["KT_hi[1]"]) and np.array_equal(cat[:, W:2 * W], g["UT_hi[1]"])
    assert np.array_equal(cat[:, 2 * W:4 * W], cat[:, :2 * W]) and np.array_equal(cat[:, 5 * W:], g["UT_lo[1]"])


def test_gates_swapped_in_ktp(clean):
    params, g = clean
    g = _copy(g)
    u = 37
    g["KTp[1]"][[u * 4 + 1, u * 4 + 2]] = g["KTp[1]"][[u * 4 + 2, u * 4 + 1]]      # gates f and c of one unit
    e = _fails(params, g)
    assert e.named == {("KTp", 1)} and e.failures[0][2] == u * 4 + 1, e.failures


def test_lo_of_the_previous_weights(clean):
    params, g = clean
    old = D.build_exact(SH, D.random_params(SH, 12), PREC)
    for key, name in (("UT_lo[1]", "UT_lo"), ("KT_lo[0]", "KT_lo"), ("E_lo", "E_lo")):
        e = _fails(params, dict(g, **{key: old[key]}))
        assert e.arrays == {name}, (key, e.failures)
    # ... all of them at once, and the planes the precision does not write are not asserted on
    stale = dict(g, **{k: old[k] for k in g if "_lo" in k})
    assert _fails(params, stale).arrays == {"UT_lo", "KT_lo", "E_lo"}
    D.compare(SH, params, PREC, D.ALL_GROUPS & ~D.LO, stale)


def test_et_padding_column_not_zero(clean):
    params, g = clean
    g = _copy(g)
    g["ET"][9, V] = 0x3F80
    e = _fails(params, g)
    assert e.arrays == {"ET"} and e.failures[0][2:4] == (9, V), e.failures


def test_ek_row_repeated(clean):
    params, g = clean
    g = _copy(g)
    g["EK"][V - 1] = g["EK"][V - 2]
    e = _fails(params, _downstream(g, params))
    assert e.arrays == {"EK"} and e.failures[0][2] == V - 1, e.failures


def test_ek_small_row_is_held_to_its_own_maximum():
    """a character whose embedding is 1e-3 of the others': a wrong row of it is 1e-3 of the array's maximum -- inside the
    array bound's reach only through the row bound"""
    params = D.random_params(SH, 13)
    D.weights(SH, params)["E"][2] *= 1e-3           # (a view into params)
    g = D.build_exact(SH, params, PREC)
    D.compare(SH, params, PREC, D.ALL_GROUPS, g)
    g["EK"][2] *= np.float32(1.01)
    e = _fails(params, _downstream(g, params))
    assert e.arrays == {"EK"} and "row bound" in e.failures[0][4] and e.failures[0][2] == 2, e.failures


def test_ctxk1_with_ctxk0s_rows(clean):
    params, g = clean
    g = _copy(g)
    g["CtxK[1]"] = D.ctxk_reference(SH, D.weights(SH, params), 1, k_rows_of=0)[0].astype(np.float32)
    e = _fails(params, _downstream(g, params))
    assert e.named == {("CtxK", 1)}, e.failures


def test_bias_missing_from_one_gate_of_ekp(clean):
    params, g = clean
    g = _copy(g)
    ekp = D.ekp_from(g["EK"], D.weights(SH, params)["b0"], W).reshape(V, W, 4)
    ekp[:, :, 3] = g["EK"][:, 3 * W:]                # gate o without b_0
    e = _fails(params, _downstream(g, params, ekp.reshape(V, 4 * W)))
    assert e.arrays == {"EKp"} and e.failures[0][2:4] == (0, 3), e.failures


def test_fragment_lane_quarters_exchanged(clean):
    params, g = clean
    g = _copy(g)
    f = g["UF[1]"]
    f[5, 1, 0, 16:32], f[5, 1, 0, 32:48] = f[5, 1, 0, 32:48].copy(), f[5, 1, 0, 16:32].copy()      # quarters 1 and 2 of one block
    e = _fails(params, g)
    assert e.named == {("UF", 1)} and e.failures[0][2:4] == (5 * 16, 32 + 8), e.failures


def test_one_tile_of_un_stale(clean):
    params, g = clean
    old = D.build_exact(SH, D.random_params(SH, 12), PREC)
    g = _copy(g)
    g["Un[1]"][0:64, 128:192] = old["Un[1]"][0:64, 128:192]
    e = _fails(params, g)
    assert e.named == {("Un", 1)} and e.failures[0][2] == 0 and 128 <= e.failures[0][3] < 192, e.failures


def test_wtcat_second_block_holds_lo(clean):
    params, g = clean
    g = _copy(g)
    g["WTcat[1]"][:, 2 * W:4 * W] = g["WTcat[1]"][:, 4 * W:]
    e = _fails(params, g)
    assert e.named == {("WTcat", 1)} and e.failures[0][3] == 2 * W, e.failures
    # (bf16 precision writes the first block only: the same array is then not asserted on beyond it)
    gb = D.build_exact(SH, params, D.PREC_BF16)
    gb["WTcat[1]"][:, 2 * W:] = 0x7FC0
    D.compare(SH, params, D.PREC_BF16, D.ALL_GROUPS & ~D.LO, gb)


def test_comb_row_from_the_next_context_value(clean):
    params, g = clean
    g = _copy(g)
    v, c = 3, R - 1                                  # (v, c + 1) is then the next character's first row
    g["comb"][v * R + c] = g["comb"][v * R + c + 1]
    e = _fails(params, g)
    assert e.arrays == {"comb"} and e.failures[0][2] == v * R + c, e.failures


def test_groups_not_current_are_not_compared(clean):
    params, g = clean
    g = _copy(g)
    g["UF[0]"][:] = 0
    g["WTperm[0]"][:] = 0
    g["comb"][:] = 0
    D.compare(SH, params, PREC, D.EAGER | D.LO | D.INTERLEAVED, g)
    assert _fails(params, g).arrays == {"UF", "WTperm", "comb"}


def test_reader_round_trip(clean):
    """read_derived finds in a byte buffer what a view describes: every carved array, in the definition's shape"""
    params, g = clean

    class View:
        pass
    v = View()
    v.depth, v.width, v.voc_size, v.Vp, v.n_ctx, v.ctx_vocab, v.ctx_dim = SH.depth, W, V, Vp, SH.n_ctx, R, SH.ctx_dim
    v.has_comb, v.mask_il, v.mask_KF = 1, 0b10, 0b10
    per_layer = ("UT_hi", "UT_lo", "KT_hi", "KT_lo", "Un", "Kn", "KTp", "bp", "UF", "KF", "WTcat", "WTperm")
    for n in per_layer + ("CtxK", "CtxKp"):
        setattr(v, "off_" + n, [0] * 16)
    chunks, off = [], 0

    def put(a):
        nonlocal off
        start = off
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        pad = (-b.size) % 256
        chunks.append(np.concatenate([b, np.full(pad, 0xAB, dtype=np.uint8)]))
        off += b.size + pad
        return start
    put(np.zeros(256, dtype=np.uint8))
    for key, a in g.items():
        name, _, idx = key.partition("[")
        if name in ("UF", "KF", "EF"):               # carved for two planes
            a = a.reshape(-1)
        if idx:
            getattr(v, "off_" + name)[int(idx[:-1])] = put(a)
        else:
            setattr(v, "off_" + name, put(a))
    v.bytes = off
    sh, got = D.read_derived(v, np.concatenate(chunks))
    assert set(got) == set(g)
    D.compare(sh, params, PREC, D.ALL_GROUPS, got)
