"""CPU proof of tests/phase_tables.py, the reference of the GPU phase-contract tests: its
expectation builder -- the oracle's primitives strung together per layer spec -- reproduces the
oracle's own methods (which the reference goldens pin), so it is no restatement of the kernel;
its tables have the properties the GPU tests rely on; and the padding behind a caller-written
norm row could change every item-3 selection, so a kernel that read it would be caught."""
import numpy as np
import pytest

import phase_tables as PT
import prng
from oracle import oracle


def _layers(seed, shapes, dt, variant):
    return [(prng.gen_keys(seed + i, s, dt, variant), prng.gen_values(seed + i, s, dt))
            for i, s in enumerate(shapes)]


def _same(got, ref):
    for (gk, gv, _), (rk, rv, _) in zip(got, ref):
        assert gk.shape == rk.shape
        assert np.array_equal(gk.view(np.uint8), np.ascontiguousarray(rk).view(np.uint8))
        assert np.array_equal(gv.view(np.uint8), np.ascontiguousarray(rv).view(np.uint8))


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("variant", ["few", "special"])
def test_builder_reproduces_fix_size_l2(dt, variant):
    """fix_size_l2.py:99-150: zone [0, S-P), keep F-P, tail the last P; keep_low / keep_high."""
    layers = _layers(11, [(2, 2, 300, 64), (1, 3, 97, 64)], dt, variant)
    for F, r, strategy, order in ((60, 0.25, "keep_low", PT.ASC), (40, 0.0, "keep_high", PT.DESC)):
        P = int(F * r)
        got = []
        for K, V in layers:
            S = K.shape[2]
            s = PT.spec(S, 0, S - P, F - P, 0, S - P, P)
            got.append(PT.expected_layer(K, V, s, order, PT.SORT))
        _same(got, oracle.fix_size_l2_compress(layers, fix_kv_size=F, keep_ratio=r,
                                               strategy=strategy, skip_layers=[]))


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_builder_reproduces_h2o_l2(dt):
    """h2o_l2.py:99-151: sink, middle zone, recent tail; the second layer's middle is one
    position longer than the heavy-hitter budget (n_select == zone_len - 1)."""
    layers = _layers(23, [(1, 2, 400, 64), (2, 2, 75, 64)], dt, "special")
    start, hh, recent = 4, 30, 40
    got = []
    for K, V in layers:
        S = K.shape[2]
        zl = S - recent - start
        s = PT.spec(S, start, zl, min(hh, zl), start, S - recent, recent)
        got.append(PT.expected_layer(K, V, s, PT.ASC, PT.SORT))
    assert got[1][2].shape[2] == 75 - 44 - 1  # one middle position evicted
    _same(got, oracle.h2o_l2_compress(layers, start_size=start, heavy_hitter_size=hh,
                                      recent_size=recent, skip_layers=[]))


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("pool", [1, 5])
def test_builder_reproduces_snapkv_lite(dt, pool):
    """snapkv_lite.py:83-152: zone the prefix, snapkv scores (pooled or not), topk, tail the
    observation window."""
    layers = _layers(37, [(1, 2, 500, 64), (2, 2, 131, 64)], dt, "special")
    obs, keep = 16, 80
    got = []
    for K, V in layers:
        S = K.shape[2]
        s = PT.spec(S, 0, S - obs, keep - obs, 0, S - obs, obs, PT.SNAPKV, pool)
        got.append(PT.expected_layer(K, V, s, PT.DESC, PT.TOPK))
    _same(got, oracle.snapkv_lite_compress(layers, observation_window=obs, keep_size=keep,
                                           pooling_kernel=pool, skip_layers=[]))


def test_split_tables_reach_every_selection_kernel():
    """The four longest zones are the first lengths of the four selection kernels (one 64-token
    tile past each dispatch edge; 1 000 for the smallest), the tables hold the four layer kinds
    the contract names, and only the longest zone is tile-aligned."""
    assert [PT.kernel_for(z) for z in PT.SPLIT_ZONES] == [n for _, n in PT.KERNEL_EDGES]
    assert [PT.kernel_for(z - 64) for z in PT.SPLIT_ZONES[1:]] == \
        [n for _, n in PT.KERNEL_EDGES[:3]]
    for Z in PT.SPLIT_ZONES:
        t = PT.split_table(Z)
        assert max(s["zone_len"] for s in t) == Z
        assert (t[1]["n_select"], t[1]["sink"], t[1]["tail_len"]) == (0, 3, 5)
        assert t[2]["n_select"] == t[2]["zone_len"] > 0
        for s in (t[0], t[3]):
            assert 0 < s["n_select"] < s["zone_len"] and s["sink"] > 0 and s["tail_len"] > 0
        assert t[0]["n_select"] * 64 > t[0]["zone_len"]    # introselect
        assert t[3]["n_select"] * 64 <= t[3]["zone_len"]   # heap select
        assert [s["zone_len"] % 64 != 0 for s in t[1:]] == [True] * 3
    assert len(PT.split_cases()) == 37 and len(PT.snapkv_cases()) == 8
    # snapkv tables: NaN norms take part in batch 0 of layer 3 (every score of such a row is
    # NaN), batch 1 has none and so can tell a wrong scoring
    for Z, dt, pool in PT.snapkv_cases():
        s = PT.split_table(Z, PT.SNAPKV, pool)[3]
        B, H = PT.split_geometry(Z)
        K = PT.gen_keys(s, B, H, 64, dt)
        nrm = oracle.as_float(oracle.norms(K[:, :, s["zone_start"]:s["zone_start"] + s["zone_len"]]))
        assert B == 2 and np.isnan(nrm[0]).any(axis=-1).all() and not np.isnan(nrm[1]).any()


def test_chunk_tables_straddle_the_argument_chunks():
    for n in (65, 129):
        t = PT.chunk_table(n)
        tiles = np.cumsum([0] + [-(-s["zone_len"] // 64) for s in t])
        assert all(0 < s["n_select"] < s["zone_len"] for s in t)
        assert all(s["zone_len"] % 64 for s in t)
        assert tiles[64] == 170 and (n < 129 or tiles[128] == 340)


def test_norm_inputs_cover_both_sides_of_every_edge():
    """One length to either side of every dispatch edge, n_select on both sides of topk's
    k * 64 <= n wherever the row is long enough; zone_len 1 leaves nothing to decide (no
    0 < n_select < 1), so it contributes no input."""
    assert PT.norm_selects(1) == [] and PT.norm_selects(2) == [1]
    for n in PT.NORM_ZONES[3:]:  # from 64 positions on
        ks = PT.norm_selects(n)
        assert any(k * 64 <= n for k in ks) and any(k * 64 > n for k in ks), n
    for edge in (64, 8192, 16384, 65536):
        assert {edge - 1, edge, edge + 1} <= set(PT.NORM_ZONES)
    for n, dt, pair, k, o, a in PT.norm_inputs():
        vals = PT.norm_rows(n, dt, pair) if k == PT.norm_selects(n)[0] and o == PT.ASC else None
        if vals is None:
            continue
        f = oracle.as_float(vals)
        assert vals.shape == (1, 2, n)
        assert not (f < 0).any() and not np.isneginf(f).any()  # what a norm can be
    f = oracle.as_float(PT.norm_rows(8191, "bf16", 2))[0, 0]
    assert (f > 0).all() and (f < 2.0 ** -126).all()  # sub-normal in bf16 and fp32
    assert len(np.unique(oracle.as_float(PT.norm_rows(8191, "bf16", 0))[0, 1])) == 8


def test_padding_could_change_every_selection():
    """For every item-3 input whose zone is no multiple of 64 (the row then has padding inside
    its last 16-byte vector and tile), selecting with ONE padding column included gives another
    set for at least one padding value, in both rows.  Inputs where it does not are listed in
    NORM_DROPPED and left out on the GPU: at most 10 % of them."""
    inputs = [i for i in PT.norm_inputs() if i[0] % 64]
    rows = {}
    fails = set()
    for inp in inputs:
        key = inp[:3]
        if key not in rows:
            rows.clear()
            rows[key] = PT.norm_rows(*key)
        if not PT.padding_matters(inp, rows[key]):
            fails.add(inp)
    print(f"item-3 inputs: {len(PT.norm_inputs())}, with padding: {len(inputs)}, "
          f"padding-insensitive: {sorted(fails)}")
    assert fails == set(PT.NORM_DROPPED)
    assert len(fails) * 10 <= len(inputs)
    assert not any(i in PT.NORM_DROPPED for i in PT.norm_cases())
