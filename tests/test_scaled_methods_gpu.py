"""Per-token-scaled fp8 paged caches through compress_paged: every method (and evict_for_space),
both formats, D = 64 / 128, single-length layers of 600 and 1 500 rows and one ragged call, against
scaled_util's expectation -- the oracle on surrogate keys that carry the contract's stored norms,
the K / V bytes and the K / V scale words taken at the kept positions.  Every check compares the
WHOLE K, V, K-scale and V-scale backings with a snapshot that has the expected rows and words
written in through the table: the result and every byte that must not change (rows past n_out,
spare pages, the poison padding of the strided scale pools) in one comparison, plus the returned
lengths."""
import numpy as np
import pytest
import torch

import fp8_gpu as G
import fp8_util as F
import prng
import scaled_gpu as SG
import scaled_util as SU
from gpu_util import to_dev
from kvcompress import _engine as E
from kvcompress import compress_paged
from oracle import oracle

pytestmark = pytest.mark.gpu
NAMES = tuple(F.METHODS) + ("evict_for_space",)


def _bytes(t):
    return t.clone(memory_format=torch.contiguous_format).reshape(-1).view(torch.uint8)


def _split(layer):
    """A [B, H, S, ...] layer as B single sequences."""
    return [tuple(x[b:b + 1] for x in layer) for b in range(layer[0].shape[0])]


def _pools(layers, fmt, P, seed, **kw):
    return [SG.ScaledPool(_split(l), fmt, P, seed + 13 * i,
                          G.STORAGES[i % 2], SG.SCALE_STORAGES[i % 2], **kw)
            for i, l in enumerate(layers)]


def _norms(layer, fmt, k_mode="pool", uniform=None):
    k8, ks = layer[0], layer[2]
    return SU.stored_norms(k8, ks if k_mode == "pool" else
                           np.float32(uniform) if k_mode == "uniform" else None, fmt)


def _expect_and_check(method, kw, layers, pools, fmt, ctx, norms=None, pos=None):
    """Run compress_paged on single-length scaled pools and compare lengths and whole pools."""
    if pos is None:
        norms = [_norms(l, fmt) for l in layers] if norms is None else norms
        pos = SU.kept_positions(SU.ORACLE_FNS[method], norms, **kw)
    snaps = [p.snapshot() for p in pools]
    before = [p.snapshot() for p in pools]
    lens = compress_paged(method, [p.paged() for p in pools], **kw)
    torch.cuda.synchronize()
    assert list(lens) == [p_.shape[2] for p_ in pos], ctx + ("lengths", lens)
    moved = False
    for li, (pool, snap, p_, l) in enumerate(zip(pools, snaps, pos, layers)):
        wk, wv, sk, sv = SU.expected_layer(p_, *l)
        for b in range(p_.shape[0]):
            pool.expect(snap, b, wk[b:b + 1], wv[b:b + 1], sk[b:b + 1], sv[b:b + 1])
        pool.assert_pools(snap, ctx + (li,))
        moved |= any(pool.changed(before[li]))
    return lens, pos, moved


def _calls(method):
    kw = SU.KWARGS[method]
    return [kw] + ([dict(kw, skip_layers=[0])] if "skip_layers" in kw else [])


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("method", NAMES)
def test_every_method_on_single_length_layers(method, fmt, D):
    """Two layers (600 and 1 500 rows, H = 2, P = 16), and once more with layer 0 skipped for the
    methods that take a skip list."""
    layers = SU.method_layers(92000 + D, D, fmt)
    for kw in _calls(method):
        pools = _pools(layers, fmt, 16, 93000)
        _, _, moved = _expect_and_check(method, kw, layers, pools, fmt, (method, fmt, D, str(kw)))
        assert moved  # the expectation is not the untouched pools


@pytest.mark.parametrize("P", (1, 64))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_fix_size_l2_other_page_sizes(fmt, P):
    for D in (64, 128):
        layers = SU.method_layers(92500 + D, D, fmt)
        _expect_and_check("fix_size_l2", SU.KWARGS["fix_size_l2"], layers,
                          _pools(layers, fmt, P, 93500 + P), fmt, ("fix_size_l2", fmt, D, P))


def test_33_layers_cross_the_argument_chunk():
    """33 scaled layers compacted in place in one launch: the argument chunk of a paged launch
    holds 32.  (D = 64: the narrowest fp8 row.)"""
    fmt, D, kw = "e4m3", 64, dict(SU.KWARGS["fix_size_l2"], fix_kv_size=48)
    layers = SU.method_layers(92700, D, fmt, lens=(100,) * 33)
    lens, _, moved = _expect_and_check("fix_size_l2", kw, layers, _pools(layers, fmt, 16, 93700),
                                       fmt, ("33 layers",))
    assert list(lens) == [48] * 33 and moved


def _ragged_layers(seed, D, fmt, n_layers=2):
    return [[SU.method_layer(seed + 100 * l + b, n, D, fmt) for b, n in enumerate(SU.RAGGED_LENS)]
            for l in range(n_layers)]


def _ragged_expect(method, kw, layers, fmt):
    """pos[l][b]: the kept positions of sequence b's layers alone."""
    L, B = len(layers), len(layers[0])
    pos = [[None] * B for _ in range(L)]
    for b in range(B):
        norms = [_norms(layers[l][b], fmt) for l in range(L)]
        out = SU.kept_positions(SU.ORACLE_FNS[method], norms, **kw)
        for l in range(L):
            pos[l][b] = out[l]
    return pos


def _ragged_check(method, kw, layers, fmt, ctx):
    pos = _ragged_expect(method, kw, layers, fmt)
    pools = [SG.ScaledPool(l, fmt, 16, 95000 + i, G.STORAGES[i % 2], SG.SCALE_STORAGES[i % 2])
             for i, l in enumerate(layers)]
    snaps = [p.snapshot() for p in pools]
    lens = compress_paged(method, [p.paged(ragged=True) for p in pools], **kw)
    torch.cuda.synchronize()
    for l, (pool, snap) in enumerate(zip(pools, snaps)):
        assert list(lens[l]) == [p_.shape[2] for p_ in pos[l]], ctx + (l, lens[l])
        for b, p_ in enumerate(pos[l]):
            pool.expect(snap, b, *SU.expected_layer(p_, *layers[l][b]))
        pool.assert_pools(snap, ctx + (l,))


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("method", NAMES)
def test_every_method_in_one_ragged_call(method, fmt, D):
    """Lengths 0 / 37 / 512 / 513 / 1 500 in one call, two layers, and once more with layer 0
    skipped for the methods that take a skip list."""
    layers = _ragged_layers(94000 + D, D, fmt)
    for kw in _calls(method):
        _ragged_check(method, kw, layers, fmt, (method, fmt, D, str(kw)))


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_fix_size_l2_at_d256(fmt):
    """The NC = 16 instances of the scaled SCORE and GATHER kernels, single-length and ragged."""
    kw = SU.KWARGS["fix_size_l2"]
    layers = SU.method_layers(94700, 256, fmt)
    _, _, moved = _expect_and_check("fix_size_l2", kw, layers, _pools(layers, fmt, 16, 94800), fmt,
                                    ("fix_size_l2", fmt, 256))
    assert moved
    _ragged_check("fix_size_l2", kw, _ragged_layers(94900, 256, fmt), fmt, ("ragged", fmt, 256))


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_ragged_call_equals_the_single_sequence_calls(fmt):
    D, method, kw = 128, "fix_size_l2", SU.KWARGS["fix_size_l2"]
    layers = _ragged_layers(94500, D, fmt)
    pools = [SG.ScaledPool(l, fmt, 16, 95500 + i) for i, l in enumerate(layers)]
    rag = [p.paged(ragged=True) for p in pools]
    lens = compress_paged(method, rag, **kw)
    for b, n in enumerate(SU.RAGGED_LENS):
        single = [SG.ScaledPool([l[b]], fmt, 16, 96000 + i) for i, l in enumerate(layers)]
        one = [p.paged() for p in single]
        lens1 = compress_paged(method, one, **kw)
        torch.cuda.synchronize()
        for l in range(len(layers)):
            n_out = lens[l][b]
            assert lens1[l] == n_out, (fmt, b, l)
            for x, y in zip(rag[l].to_dense(n_out, b) + rag[l].scales_to_dense(n_out, b),
                            one[l].to_dense(n_out) + one[l].scales_to_dense(n_out)):
                assert torch.equal(_bytes(x), _bytes(y)), (fmt, b, l)


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_uniform_absent_and_mixed_layers(fmt):
    """One call of four layers: per-token K with a uniform V scale; per-token K with no V scale;
    a uniform K scale with per-token V scales (the V words still follow the rows); and an unscaled
    layer.  Uniform words and their poison neighbours are never written."""
    D, method, kw = 128, "fix_size_l2", SU.KWARGS["fix_size_l2"]
    layers = SU.method_layers(97000, D, fmt, lens=(600, 700, 800, 900))
    modes = [dict(v_mode="uniform", uniform=(None, 2.5)), dict(v_mode="none"),
             dict(k_mode="uniform", uniform=(0.37, None)), dict(k_mode="none", v_mode="none")]
    pools = [SG.ScaledPool(_split(l), fmt, 16, 97500 + i, **m)
             for i, (l, m) in enumerate(zip(layers, modes))]
    paged = [p.paged() for p in pools]
    assert [p.scaled for p in paged] == [True, True, True, False]
    norms = [_norms(l, fmt, m.get("k_mode", "pool"), (m.get("uniform") or (None,))[0])
             for l, m in zip(layers, modes)]
    pos = SU.kept_positions(SU.ORACLE_FNS[method], norms, **kw)
    snaps = [p.snapshot() for p in pools]
    lens = compress_paged(method, paged, **kw)
    torch.cuda.synchronize()
    assert list(lens) == [p_.shape[2] for p_ in pos]
    for li, (pool, snap, p_, l) in enumerate(zip(pools, snaps, pos, layers)):
        pool.expect(snap, 0, *SU.expected_layer(p_, *l))
        pool.assert_pools(snap, (fmt, li))
    # the unscaled layer is the unscaled fp8 call's result
    want = F.kept_positions(oracle.fix_size_l2_compress, [layers[3][0]], fmt, **kw)[0]
    assert np.array_equal(want, pos[3])


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_stable_policy(fmt, monkeypatch):
    monkeypatch.setattr(E, "tie_policy", "stable")
    monkeypatch.setattr(oracle, "TIE", "stable")
    layers = SU.method_layers(98200, 128, fmt)
    norms = [_norms(l, fmt) for l in layers]
    for method in ("fix_size_l2", "snapkv_lite", "h2o_l2"):
        _, pos, _ = _expect_and_check(method, SU.KWARGS[method], layers,
                                      _pools(layers, fmt, 16, 98500), fmt, (method, fmt, "stable"))
    st = SU.kept_positions(oracle.fix_size_l2_compress, norms, **SU.KWARGS["fix_size_l2"])
    monkeypatch.setattr(oracle, "TIE", "reference")
    ref = SU.kept_positions(oracle.fix_size_l2_compress, norms, **SU.KWARGS["fix_size_l2"])
    assert any(not np.array_equal(a, b) for a, b in zip(ref, st))  # the policies differ here


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_random_strategy_scales_follow_caller_indices(fmt):
    """strategy="random": the indices are the caller's (a seeded draw).  The same draw on dense
    bf16 tensors with position-encoding V gives the positions; rows and scale words follow them."""
    from kvcompress.methods import fix_size_l2_compress
    D = 64
    kw = dict(fix_kv_size=256, keep_ratio=0.25, strategy="random", skip_layers=[])
    layers = SU.method_layers(99000, D, fmt)
    dense = [(to_dev(prng.gen_keys(1, l[0].shape, "bf16"), G.DEV),
              to_dev(prng.encode_positions(l[0].shape, "bf16"), G.DEV)) for l in layers]
    torch.manual_seed(321)
    out = fix_size_l2_compress(dense, **kw)
    pos = []
    for _, v in out:
        bits = v.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        p_, ok = prng.decode_positions(bits, "bf16")
        assert ok
        pos.append(p_)
    assert not np.array_equal(pos[0][0, 0], pos[0][0, 1])
    torch.manual_seed(321)
    _expect_and_check("fix_size_l2", kw, layers, _pools(layers, fmt, 16, 99500), fmt,
                      (fmt, "random"), pos=pos)


def test_status_check_stays_quiet(monkeypatch):
    monkeypatch.setattr(E, "check_status", True)
    for fmt in F.FORMATS:
        layers = SU.method_layers(99700, 64, fmt)
        _expect_and_check("snapkv_lite", SU.KWARGS["snapkv_lite"], layers,
                          _pools(layers, fmt, 16, 99800), fmt, (fmt, "status check"))


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_captured_call_replays_over_refilled_pools(fmt):
    """One scaled in-place call captured after an eager warm-up and replayed over refilled K, V
    and scale pools (same tensors, new contents): every replay is the expectation of its fill."""
    D, method, kw = 128, "fix_size_l2", SU.KWARGS["fix_size_l2"]
    fills = [SU.method_layers(100000 + 50 * f, D, fmt) for f in range(3)]
    pools = _pools(fills[0], fmt, 16, 100500)
    paged = [p.paged() for p in pools]
    clean = [p.snapshot() for p in pools]

    def refill(layers):
        snaps = []
        for pool, c, l in zip(pools, clean, layers):
            for back, src in zip((pool.kb, pool.vb) + tuple(pool.sb), c):
                back.copy_(src)
            wk = tuple(SU.words(x) for x in l[2:])
            pool.expect((pool.kb, pool.vb) + tuple(pool.sb), 0, l[0], l[1], *wk)
            snaps.append(pool.snapshot())
        return snaps

    def check(layers, snaps, what):
        torch.cuda.synchronize()
        pos = SU.kept_positions(SU.ORACLE_FNS[method], [_norms(l, fmt) for l in layers], **kw)
        for li, (pool, snap, p_, l) in enumerate(zip(pools, snaps, pos, layers)):
            pool.expect(snap, 0, *SU.expected_layer(p_, *l))
            pool.assert_pools(snap, (fmt, what, li))

    snaps = refill(fills[0])
    compress_paged(method, paged, **kw)  # the warm-up
    check(fills[0], snaps, "eager")
    refill(fills[1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lens = compress_paged(method, paged, **kw)
    assert lens == [256, 256]
    for f in (1, 2):
        snaps = refill(fills[f])
        g.replay()
        check(fills[f], snaps, f"replay {f}")
    del g
    torch.cuda.synchronize()


def test_dense_out_pair_raises_and_touches_nothing():
    fmt, D = "e4m3", 64
    layers = SU.method_layers(101000, D, fmt)
    pools = _pools(layers, fmt, 16, 101500)
    snaps = [p.snapshot() for p in pools]
    dst = tuple(torch.zeros((1, SU.METHOD_H, 600, D), dtype=torch.uint8, device=G.DEV)
                .view(F.torch_dtype(fmt)) for _ in range(2))
    with pytest.raises(TypeError, match="in place"):
        compress_paged("fix_size_l2", [p.paged() for p in pools], out=[None, dst],
                       **SU.KWARGS["fix_size_l2"])
    with pytest.raises(TypeError, match="in place"):
        compress_paged("fix_size_l2", [pools[0].paged(ragged=True)], out=[dst],
                       **SU.KWARGS["fix_size_l2"])
    torch.cuda.synchronize()
    for pool, snap in zip(pools, snaps):
        pool.assert_pools(snap, ("dense out",))
    assert not dst[0].view(torch.uint8).any() and not dst[1].view(torch.uint8).any()


def test_pagedkv_device_and_alignment_errors():
    from kvcompress import PagedKV
    pool = _pools(SU.method_layers(102000, 64, "e4m3"), "e4m3", 16, 102500)[0]
    ks = pool.sv[0]
    with pytest.raises(ValueError, match="is on"):
        PagedKV(pool.k, pool.v, pool.table, 600, k_scale=ks.cpu())
    with pytest.raises(ValueError, match="is on"):
        PagedKV(pool.k, pool.v, pool.table, 600, v_scale=torch.ones(1))
    with pytest.raises(TypeError, match="float32"):
        PagedKV(pool.k, pool.v, pool.table, 600, k_scale=ks.double())
    kd, vd = pool.paged().scales_to_dense()
    assert kd.shape == vd.shape == (1, SU.METHOD_H, 600)
    assert np.array_equal(kd.cpu().numpy().view(np.uint32), SU.words(
        SU.method_layers(102000, 64, "e4m3")[0][2]))
