"""The inputs of tests/test_gpu_pool_envelope.py checked with the restatement alone (no GPU): every member loads, the spiked cepstra reach the
wrap of the input quantiser for every member a GPU case gives them to, the restatement wraps as the numpy restatement of the quantiser says,
the quads widths hold mixed 4-element groups, and the member pattern holds the lists it claims.  The GPU tests rely on these checks."""
import numpy as np
import pytest

import pool_envelope_testlib as E
from kws_testlib import OracleModel
from pool_testlib import KWS_NN_WAVES, POOL_NONE, items_and_rows

B_CEP = 64


@pytest.fixture(scope="module")
def members(oracle, tmp_path_factory):
    """width -> (names, [oracle model], [(scale, zero point)]) of the mixed pool plus the two graphs outside the shape; loaded once"""
    directory = tmp_path_factory.mktemp("pool_envelope_host")
    made = {}

    def get(width):
        if width not in made:
            names = E.member_names(width) + list(E.OUTSIDE)
            paths = E.write_members(directory, width, names)
            made[width] = (names, [OracleModel(oracle, p) for p in paths], [E.input_quant(open(p, "rb").read()) for p in paths])
        return made[width]

    return get


@pytest.fixture(scope="module")
def spiked(oracle):
    """width -> the standardised rows [B_CEP][49 ncep] of the spiked cepstra (Oracle.cmvnw), once"""
    made = {}

    def get(width):
        if width not in made:
            m = E.spiked_cepstra(B_CEP, E.WIDTHS4[width]["ncep"], E.SPIKE[width])
            f = np.stack([oracle.cmvnw(x, E.WIN).reshape(-1) for x in m])
            f.setflags(write=False)
            made[width] = f
        return made[width]

    return get


def test_the_tables_are_what_they_say():
    assert [len(E.edge_keys(w)) for w in E.WIDTHS4] == [74, 0, 0, 17]
    assert [len(E.member_names(w)) for w in E.WIDTHS4] == [83, 9, 9, 26]
    assert all(E.in_mfma_shape(c["blocks"]) for c in E.CORNERS.values()) and not any(E.in_mfma_shape(c["blocks"]) for c in E.OUTSIDE.values())
    assert sorted(c["n_labels"] for c in E.CORNERS.values()) == [1, 2, 4, 7, 33, 48]
    for w, (cp, quads) in E.KERNEL_FORM.items():
        ncep = E.WIDTHS4[w]["ncep"]
        assert cp == (16 if (ncep + 15) // 16 * 16 == 16 else 64) and quads == (ncep % 4 == 0)
    assert sorted(E.KERNEL_FORM.values()) == [(16, False), (16, True), (64, False), (64, True)]
    for w in ("49x13", "49x40"):
        names = E.bank_names(w)
        assert len(names) == len(set(names)) == 16 and names[:6] == list(E.CORNERS) and set(names[6:]) <= set(E.edge_keys(w))
    assert {"g2/labels/48", "g2/labels/33"} <= set(E.bank_names("49x13"))
    seeds = [s for t in E._SEEDS.values() for s in t.values()]
    assert len(seeds) == len(set(seeds))


@pytest.mark.parametrize("width", list(E.WIDTHS4))
def test_every_member_loads_with_its_shape(width, members):
    names, oms, quant = members(width)
    ncep = E.WIDTHS4[width]["ncep"]
    for n, om in zip(names, oms):
        assert om.n_features == E.N_FRAMES * ncep and om.cfg.num_cepstral == ncep and om.cfg.win_size == E.WIN, n
        assert om.cfg.num_filters == oms[0].cfg.num_filters and om.cfg.low_frequency == oms[0].cfg.low_frequency, n
    labels = dict(zip(names, (om.n_labels for om in oms)))
    assert [labels[c] for c in E.CORNERS] == [c["n_labels"] for c in E.CORNERS.values()]
    assert max(labels[n] for n in E.member_names(width)) == 48
    # the corners' thresholds are inside what a spike gives (the rule their seeds were searched by)
    for n, (scale, zp) in zip(names, quant):
        if n in E.CORNERS or n in E.OUTSIDE:
            hi, lo = E.wrap_thresholds(scale, zp)
            assert hi <= E.THRESHOLD_MAX and lo >= -E.THRESHOLD_MAX and E.wrap_sides(scale, zp) == (True, True), (n, hi, lo)


def test_standardised_values_stay_inside_the_bound(spiked, oracle):
    """the reasoning of the testlib's docstring, measured: no displacement takes a standardised value past Z_BOUND"""
    for width in E.WIDTHS4:
        assert np.abs(spiked(width)).max() < E.Z_BOUND
    far = np.stack([oracle.cmvnw(x, E.WIN) for x in E.spiked_cepstra(4, 13, 4.0e6)])
    assert 7.0 < np.abs(far).max() <= np.float32(E.Z_BOUND) * np.float32(1.0 + 1e-6)
    at = np.abs(E.spiked_cepstra(1, 40, 40.0)[0]) > 20.0
    assert at.sum() == 40 and (at.sum(axis=0) == 1).all() and not at[E.N_FRAMES // 2].any()


@pytest.mark.parametrize("width", list(E.WIDTHS4))
def test_spiked_rows_wrap_for_every_member(width, members, spiked):
    """every member of the pool and both graphs outside the shape, on all 64 rows (a GPU case gives a member a subset of them): a value above
    127 and one below -128 before the cast on every side the member can reach, and the restatement's int8 is the wrap of that value"""
    names, oms, quant = members(width)
    f = spiked(width)
    wrapped, both = {}, 0
    for n, om, (scale, zp) in zip(names, oms, quant):
        wrapped[n] = E.assert_rows_wrap(f, scale, zp, (width, n)) / f.shape[0]
        both += E.wrap_sides(scale, zp) == (True, True)
        u = E.unwrapped(f, scale, zp)
        for i in range(f.shape[0]):
            assert (om.quantize_input(f[i]) == E.wrap(u[i])).all(), (width, n, i)
    print(width, "wrapped elements per row of %d:" % f.shape[1], {n: round(v, 1) for n, v in wrapped.items() if "/" not in n},
          "edge models %.1f .. %.1f" % (min([v for n, v in wrapped.items() if "/" in n] or [0]), max([v for n, v in wrapped.items() if "/" in n] or [0])))
    # every corner and tenants 0 and 1 wrap on both sides; what cannot (a threshold beyond Z_BOUND) is known by name
    one_sided = {n for n, (scale, zp) in zip(names, quant) if E.wrap_sides(scale, zp) != (True, True)}
    assert not one_sided & (set(E.CORNERS) | set(E.OUTSIDE) | {"tenant0", "tenant1"}), one_sided
    if width == "49x13":
        assert one_sided == {"tenant2", "g2/c0/rollover", "g2/c0/rollover+sparse", "g2/c0/in_zp_m128", "g2/c0/in_zp_p127"}, one_sided
    if width == "49x40":
        # the g2w models' drawn input scale (0.0599, zero point -4) puts both thresholds beyond the bound: they run on spiked rows that
        # do not wrap for them; the two zero-point edits wrap on one side on every row
        assert one_sided == {"tenant2"} | set(E.edge_keys(width)), one_sided
        assert [E.wrap_sides(*q) for n, q in zip(names, quant) if n.endswith("in_zp_m128") or n.endswith("in_zp_p127")] == [(False, True), (True, False)]
    assert both >= 8
    # against constant scores: the corners' scores move over the spiked rows (the rule their seeds were searched by)
    for n in list(E.CORNERS) + list(E.OUTSIDE):
        scores = np.stack([oms[names.index(n)].run_inference(x) for x in f])
        assert len(np.unique(scores, axis=0)) >= E.DISTINCT_MIN[n], (width, n, len(np.unique(scores, axis=0)))


@pytest.mark.parametrize("width", list(E.WIDTHS4))
def test_a_quantiser_that_clamped_would_show_in_the_scores(width, members, spiked):
    """what makes the GPU comparison on the spiked rows a test of the wrap: through the restatement's network, the clamped tensor gives other
    scores than the wrapped one on at least half of the 64 rows for every corner with more than one label (measured: 35 .. 64 rows)"""
    names, oms, quant = members(width)
    f = spiked(width)
    for n in E.CORNERS:
        om, (scale, zp) = oms[names.index(n)], quant[names.index(n)]
        u = E.unwrapped(f, scale, zp)
        wrapped = np.stack([om.dequantize(om.nn_invoke(E.wrap(x))) for x in u])
        assert (wrapped == np.stack([om.run_inference(x) for x in f])).all(), (width, n)
        clamped = np.stack([om.dequantize(om.nn_invoke(np.clip(x, -128, 127).astype(np.int8))) for x in u])
        changed = int((wrapped != clamped).any(axis=1).sum())
        assert changed >= (0 if om.n_labels == 1 else 32), (width, n, changed)


@pytest.mark.parametrize("width", ["49x16", "49x40"])
def test_quads_hold_wrapped_and_unwrapped_values_together(width, members, spiked):
    names, _, quant = members(width)
    f = spiked(width)
    for n, (scale, zp) in zip(names, quant):
        if E.wrap_sides(scale, zp) != (False, False):
            assert all(E.mixed_quads(f[i], E.WIDTHS4[width]["ncep"], scale, zp) >= 1 for i in range(f.shape[0])), (width, n)


def test_the_member_pattern_holds_the_lists_it_claims():
    for width in E.WIDTHS4:
        names = E.member_names(width)
        K = len(names)
        for item_rows in (4, 16, 64):
            m = E.member_pattern(names, item_rows, seed=K)
            assert (m[6::7] == POOL_NONE).all() and (m == POOL_NONE).sum() == m.size // 7
            items, rows = items_and_rows(m, K, item_rows)
            per = lambda n: [c for k, _, c in items if k == names.index(n)]
            assert per("odd") == [item_rows] and per("max") == [item_rows, 1] and per("min") == [KWS_NN_WAVES - 1]
            assert all(sum(per(n)) == KWS_NN_WAVES for n in names if n not in ("max", "odd", "min"))
            assert sorted(rows) == [i for i in range(m.size) if m[i] != POOL_NONE] and list(m[m != POOL_NONE]) != sorted(m[m != POOL_NONE])
            r = E.reversed_members(m, K)
            assert ((r == POOL_NONE) == (m == POOL_NONE)).all() and all(names[::-1][int(a)] == names[int(b)] for a, b in zip(r, m) if b != POOL_NONE)
        assert E.member_pattern(names, 16, seed=K).size <= 420
        calls = E.cepstra_calls(K, B_CEP)
        seen = np.concatenate([E.cepstra_members(K, B_CEP, c) for c in range(calls)])
        assert set(range(K)) <= set(int(x) for x in seen) and (seen.reshape(calls, B_CEP)[:, 6::7] == POOL_NONE).all()
