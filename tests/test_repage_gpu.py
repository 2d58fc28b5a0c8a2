"""Paged destinations on the GPU (include/kvc.h, "Paged destinations"; kvcompress.PagedDest):
the compressed sequence of a paged layer written through a second block table into fresh pages of
the same pool or into another pool, the source pool only read.

Expected bytes come from the CPU oracle (tests/dest_cases.py, tests/ragged_util.py,
tests/scaled_util.py).  Every check compares WHOLE backing buffers with a snapshot that has the
expected rows written in through the destination table (tests/repage_util.py): the result, the
untouched source pages, the spare pages and the poison around the written rows in one comparison.
That comparisons of this form cannot pass with the destination table ignored or misread is shown on
the CPU in tests/test_repage_model.py (on case 1's own data and on synthetic data shaped like
cases 3, 6 and 7).

A destination pool is the source's own view or byte-disjoint from it (compress_paged checks it), so
"fresh pages of the same pool" has the source's page size: the cases with a destination page size
of 4 or 64 beside a source of 16 go into a pool of their own.
"""
import numpy as np
import pytest
import torch

import dest_cases as DC
import paged_util as PU
import prng
import ragged_util as RU
import repage_util as RP
from gpu_util import to_dev, to_np
from kvcompress import _native as N

pytestmark = pytest.mark.gpu

DEV = PU.DEV


def _policy(monkeypatch, case):
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "tie_policy", case["tie"])


def _expected(layers, ref):
    """[(K rows, V rows)] of every layer: the oracle's result, the input itself where the method
    left the layer alone (it is delivered all the same)."""
    return [(k, v) if kind == "same" else (rk, rv) for (k, v), (rk, rv, kind) in zip(layers, ref)]


def _run_single(case, Pd, separate, storages=("nhpd", "nphd"), dst_storages=("nhpd", "nphd")):
    from kvcompress import compress_paged
    layers, ref = DC.reference(case, tagged=False)
    want = _expected(layers, ref)
    pls, dsts = [], []
    for li, ((k, v), (wk, _)) in enumerate(zip(layers, want)):
        B, H, S, D = k.shape
        n, seed = wk.shape[2], case["seed"] + 7 * li
        if separate:
            pls.append(PU.Layer(k, v, 16, seed, k_storage=storages[0], v_storage=storages[1]))
            dsts.append(RP.Dest([n] * B, Pd, seed + 1, H, D, pls[-1].k.dtype,
                                storages=dst_storages))
        else:
            with RP.spare(B * -(-n // 16)):
                pls.append(PU.Layer(k, v, 16, seed))
            dsts.append(RP.same_pool_dest(pls[-1], [n] * B, seed, B * -(-S // 16)))
    src_snaps = [pl.snapshot() for pl in pls]
    snaps = [d.snapshot() for d in dsts]
    lens = compress_paged(case["method"], [pl.paged for pl in pls],
                          out=[d.paged_dest() for d in dsts], **case["kw"])
    torch.cuda.synchronize()
    assert lens == [wk.shape[2] for wk, _ in want], (case["id"], lens)
    for li, (pl, d, snap, (wk, wv)) in enumerate(zip(pls, dsts, snaps, want)):
        ctx = (case["id"], Pd, li, ref[li][2])
        d.expect(snap, wk, wv)
        d.assert_pools(snap, ctx)
        if separate:
            pl.assert_pools(src_snaps[li], ctx + ("source unchanged",))


CASES = [(c, Pd) for c in DC.INPLACE for Pd in (4, 16, 64)]


@pytest.mark.parametrize("case, Pd", CASES, ids=[f"{c['id']}-Pd{Pd}" for c, Pd in CASES])
def test_every_method(case, Pd, monkeypatch):
    """1 (and 5: the stable-policy case is one of them): every in-place and strided-destination
    case, source P = 16, into fresh pages of the same pool (Pd = 16) or a pool of pages of 4 / 64.
    Among them a layer the method skips, one below its threshold and recent_only's slice."""
    _policy(monkeypatch, case)
    _run_single(case, Pd, separate=Pd != 16)


PER_METHOD = {}
for _c in DC.INPLACE:
    PER_METHOD.setdefault(_c["method"], _c)


@pytest.mark.parametrize("case", list(PER_METHOD.values()), ids=list(PER_METHOD))
def test_separate_pool_of_the_other_storage(case, monkeypatch):
    """2: source [N, H, P, D], destination K [N, P, H, D] and V [N, H, P, D] (K's and V's strides
    differ); the source buffers are unchanged."""
    _policy(monkeypatch, case)
    _run_single(case, 16, True, storages=("nhpd", "nhpd"), dst_storages=("nphd", "nhpd"))


def _prefix_setup(seed=43000):
    """B = 3 sequences of 600 rows whose tables share the pages of rows [0, 512)."""
    B, H, S, D, P = 3, 2, 600, 64, 16
    kn, vn = prng.gen_keys(seed, (B, H, S, D), "bf16"), prng.gen_values(seed, (B, H, S, D), "bf16")
    kn[1:, :, :512], vn[1:, :, :512] = kn[0, :, :512], vn[0, :, :512]
    shared, own, fresh = 512 // P, -(-(S - 512) // P), -(-168 // P)
    n_pages = shared + B * own + B * fresh + RP.SPARE
    perm = np.random.default_rng(seed).permutation(n_pages)
    table = np.concatenate([np.broadcast_to(perm[:shared], (B, shared)),
                            perm[shared:shared + B * own].reshape(B, own)], axis=1).astype(np.int64)
    pl = PU.Layer(kn, vn, P, 0, table=table, n_pages=n_pages)
    dst = RP.same_pool_dest(pl, [168] * B, seed, shared + B * own)
    return kn, vn, pl, dst, perm[:shared]


def test_shared_prefix_into_fresh_pages():
    """3: the motivating case -- one physical prefix under three sequences, h2o_l2 into disjoint
    fresh pages; every sequence equals the oracle on its own dense rows and the shared pages are
    unchanged (the whole-pool comparison).  check_repage_tables accepts these tables and refuses
    the same call's in-place tables."""
    from kvcompress import compress_paged
    from kvcompress.paged import check_repage_tables
    from oracle import oracle
    kn, vn, pl, dst, shared = _prefix_setup()
    kw = dict(start_size=4, heavy_hitter_size=64, recent_size=100, skip_layers=[])
    (rk, rv, _), = oracle.METHODS["h2o_l2"]([(kn, vn)], **kw)
    snap = dst.snapshot()
    lens = compress_paged("h2o_l2", [pl.paged], out=[dst.paged_dest()], **kw)
    torch.cuda.synchronize()
    assert lens == [168] and rk.shape[2] == 168
    dst.expect(snap, rk, rv)
    dst.assert_pools(snap, ("shared prefix",))
    kd, _ = pl.paged.to_dense(512)  # (explicitly: the shared pages still hold the prefix)
    assert np.array_equal(to_np(kd), kn[:, :, :512])
    check_repage_tables(pl.table_np, 600, 16, dst.table_np, 168, 16)
    with pytest.raises(ValueError, match="source page"):
        check_repage_tables(pl.table_np, 600, 16, pl.table_np, 168, 16)


def test_caller_indices():
    """4: strategy="random" (caller indices per head) and h2o_attention without a manager run
    through a PagedDest; expectations as in test_paged_gpu's in-place tests."""
    from kvcompress import compress_paged
    from kvcompress.methods import fix_size_l2_compress
    from oracle import oracle
    shape = (DC.B, DC.H, 1500, 64)
    kn, vn = prng.gen_keys(42090, shape, "bf16"), prng.encode_positions(shape, "bf16")
    with RP.spare(DC.B * 32):
        pl = PU.Layer(kn, vn, 16, 42090)
    dst = RP.same_pool_dest(pl, [512] * DC.B, 42090, DC.B * 94)
    kw = dict(fix_kv_size=512, keep_ratio=0.25, strategy="random", skip_layers=[])
    torch.manual_seed(77)
    want = fix_size_l2_compress([(to_dev(kn, DEV), to_dev(vn, DEV))], **kw)
    snap = dst.snapshot()
    torch.manual_seed(77)
    lens = compress_paged("fix_size_l2", [pl.paged], out=[dst.paged_dest()], **kw)
    torch.cuda.synchronize()
    assert lens == [512] and want[0][0].shape[2] == 512
    dst.expect(snap, to_np(want[0][0]), to_np(want[0][1]))
    dst.assert_pools(snap, ("random",))

    shape = (2, 3, 600, 64)
    layers = [(prng.gen_keys(42200 + i, shape, "bf16"), prng.gen_values(42200 + i, shape, "bf16"))
              for i in range(2)]
    with RP.spare(2 * 11):
        pls = [PU.Layer(k, v, 16, 42200 + i) for i, (k, v) in enumerate(layers)]
    dsts = [RP.same_pool_dest(pl, [168] * 2, 42200 + i, 2 * 38) for i, pl in enumerate(pls)]
    kw = dict(start_size=4, heavy_hitter_size=64, recent_size=100)
    ref = oracle.METHODS["h2o_l2"](layers, skip_layers=[], **kw)
    snaps = [d.snapshot() for d in dsts]
    lens = compress_paged("h2o_attention", [pl.paged for pl in pls],
                          out=[d.paged_dest() for d in dsts], **kw)
    torch.cuda.synchronize()
    assert lens == [168, 168]
    for d, snap, (rk, rv, _) in zip(dsts, snaps, ref):
        d.expect(snap, rk, rv)
        d.assert_pools(snap, ("h2o_attention",))


# ---- 6: ragged ------------------------------------------------------------------------------
def _ragged_setup(seed, lens, D, dtype, P, L, storages, new_max, same):
    """Ragged layers and their destinations (Pd = 16): fresh pages of the same pool when the
    source has pages of 16, else a pool of their own."""
    if same:
        with RP.spare(RP.pages_for([min(n, new_max) for n in lens], 16)):
            layers_np, pls = RU.build(seed, lens, RU.H, D, dtype, P, L, storages=storages)
        dsts = [RP.same_pool_dest(pl, [min(n, new_max) for n in lens], seed + 7 * l,
                                  RP.pages_for(lens, P)) for l, pl in enumerate(pls)]
    else:
        layers_np, pls = RU.build(seed, lens, RU.H, D, dtype, P, L, storages=storages)
        dsts = [RP.Dest([min(n, new_max) for n in lens], 16, seed + 50 + l, RU.H, D, pl.k.dtype)
                for l, pl in enumerate(pls)]
    return layers_np, pls, dsts


RAGGED = [(m, kw, L, g) for m, kw, L in RU.METHOD_CASES for g in RU.GEOMETRIES]


@pytest.mark.parametrize("method, kw, L, geo", RAGGED,
                         ids=[f"{m}-P{g[0]}-{g[1]}-D{g[2]}" for m, _, _, g in RAGGED])
def test_ragged_every_method(method, kw, L, geo):
    """Lengths 0 / 37 / 512 / 513 / 1 500 in one call against (a) the per-sequence oracle written
    through the destination table -- the passed-through sequences (0 and 37 rows, and every
    sequence of a skipped layer) ARRIVE in their destination pages -- and (b) B single-sequence
    PagedDest calls on a twin, pool byte for pool byte and in the returned lengths."""
    from kvcompress import PagedDest, PagedKV, compress_paged
    P, dtype, D, storages = geo
    args = (4100 + 17 * P, RU.LENS, D, dtype, P, L, storages, 1500, P == 16)
    layers_np, a, da = _ragged_setup(*args)
    _, w, dw = _ragged_setup(*args)
    ref = RU.oracle_per_sequence(method, kw, layers_np)
    snaps = [d.snapshot() for d in da]
    src_snaps = [pl.snapshot() for pl in a]
    got = compress_paged(method, [pl.paged for pl in a], out=[d.paged_dest() for d in da], **kw)
    torch.cuda.synchronize()
    for l in range(L):
        assert list(got[l]) == [ref[l][b][0].shape[2] for b in range(len(RU.LENS))], (l, got[l])
        for b in range(len(RU.LENS)):
            rk, rv, kind = ref[l][b]
            rk, rv = layers_np[l][b] if kind == "same" else (rk, rv)
            da[l].expect(snaps[l], rk, rv, b)
        da[l].assert_pools(snaps[l], (method, P, l))
        if not da[l].same:
            a[l].assert_pools(src_snaps[l], (method, P, l, "source unchanged"))
    for b, n in enumerate(RU.LENS):
        one = compress_paged(
            method, [PagedKV(pl.k, pl.v, pl.table[b:b + 1], n) for pl in w],
            out=[PagedDest(d.table[b:b + 1]) if d.same else
                 PagedDest(d.table[b:b + 1], d.k, d.v) for d in dw], **kw)
        assert one == [g[b] for g in got], (b, one)
    torch.cuda.synchronize()
    for l in range(L):
        for x, y in ((a[l].kb, w[l].kb), (a[l].vb, w[l].vb), (da[l].kb, dw[l].kb),
                     (da[l].vb, dw[l].vb)):
            assert torch.equal(PU.ints(x), PU.ints(y)), (method, P, l)


def test_ragged_mix_and_launch_count(monkeypatch):
    """A ragged call with an in-place layer beside PagedDest layers; and the number of
    kvc_launch_repage / kvc_launch_ragged calls is the same for B = 2 and B = 5."""
    from kvcompress import compress_paged
    kw = dict(start_size=4, heavy_hitter_size=64, recent_size=444, skip_layers=[1])
    counts = {}
    for lens in ([1500, 37], [0, 37, 512, 513, 1500]):
        layers_np, pls, dsts = _ragged_setup(4700, lens, 64, "bf16", 16, 3, ("nhpd", "nphd"), 1500,
                                             True)
        ref = RU.oracle_per_sequence("h2o_l2", kw, layers_np)
        calls = []
        snaps = [d.snapshot() for d in dsts]  # (same pools: the sources' backings)
        with monkeypatch.context() as mp:
            for name in ("launch_repage", "launch_ragged"):
                real = getattr(N, name)
                mp.setattr(N, name, lambda *a, _r=real, _n=name: calls.append(_n) or _r(*a))
            got = compress_paged("h2o_l2", [pl.paged for pl in pls],
                                 out=[dsts[0].paged_dest(), None, dsts[2].paged_dest()], **kw)
        torch.cuda.synchronize()
        counts[len(lens)] = sorted(calls)
        for l in range(3):
            assert list(got[l]) == [ref[l][b][0].shape[2] for b in range(len(lens))]
            for b in range(len(lens)):
                rk, rv, kind = ref[l][b]
                if l == 1:  # in place (and skipped: untouched)
                    assert kind == "same"
                    continue
                rk, rv = layers_np[l][b] if kind == "same" else (rk, rv)
                dsts[l].expect(snaps[l], rk, rv, b)
            dsts[l].assert_pools(snaps[l], ("mix", len(lens), l))
    assert counts[2] == counts[5] and "launch_repage" in counts[2], counts


# ---- 12: refusals ---------------------------------------------------------------------------
def test_refusals_leave_the_pools_untouched():
    from kvcompress import PagedDest, compress_paged
    shape = (2, 3, 600, 64)
    kn, vn = prng.gen_keys(43300, shape, "bf16"), prng.gen_values(43300, shape, "bf16")
    with RP.spare(2 * 11):
        pl = PU.Layer(kn, vn, 16, 43300)
    dst = RP.same_pool_dest(pl, [168] * 2, 43300, 2 * 38)
    other = RP.Dest([168] * 2, 16, 43301, 3, 64, torch.bfloat16)
    kw = dict(start_size=4, heavy_hitter_size=64, recent_size=100, skip_layers=[])
    snap, osnap = pl.snapshot(), other.snapshot()

    def refused(exc, match, out, method="h2o_l2", layers=None, **kws):
        with pytest.raises(exc, match=match):
            compress_paged(method, layers or [pl.paged], out=[out], **(kws or kw))

    refused(ValueError, "holds fewer than the 11 pages", PagedDest(dst.table[:, :10]))
    # the source pool's pages from 1 on: overlaps it without being its view
    refused(ValueError, "K destination pool overlaps the layer's K pool",
            PagedDest(dst.table, pl.k[1:], pl.v[1:]))
    refused(TypeError, "has dtype", PagedDest(other.table, other.k.half(), other.v.half()))
    refused(ValueError, "with the layer's H = 3 and D = 64",
            PagedDest(other.table, other.k[:, :2], other.v[:, :2]))
    refused(ValueError, "with the layer's H = 3 and D = 64",
            PagedDest(other.table, other.k[..., :32], other.v[..., :32]))
    rag = __import__("kvcompress").PagedKV(pl.k, pl.v, pl.table, [600, 300])
    dense = tuple(torch.zeros(2, 3, 600, 64, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    refused(TypeError, "dense out= pairs are not supported", dense, layers=[rag])
    with pytest.raises(TypeError, match="PagedDest or None"):
        compress_paged("h2o_l2", [pl.paged], out=[5], **kw)
    torch.cuda.synchronize()
    pl.assert_pools(snap, ("after refusals",))
    other.assert_pools(osnap, ("after refusals",))
    assert not dense[0].any() and not dense[1].any()


# ---- 7: scaled fp8 --------------------------------------------------------------------------
def _scaled_dest(pool, n_rows, seed):
    """Fresh pages of a scaled pool's own K / V / scale pools."""
    return RP.Dest(n_rows, pool.P, seed,
                   pool=(pool.kb, pool.vb, pool.k, pool.v) + tuple(pool.storages),
                   used=RP.pages_for(pool.lens, pool.P))


def _scaled_expect(pool, dst, snap, b, rows):
    """ScaledPool.expect through the DESTINATION table: rows, and scale words where they move."""
    was = pool.rows
    pool.rows = dst.rows
    try:
        pool.expect(snap, b, *rows)
    finally:
        pool.rows = was


def _plant(layer):
    """A NaN-payload and a negative scale among the rows every method keeps (the last ones)."""
    import scaled_util as SU
    k8, v8, ks, vs = layer
    if ks.shape[2] >= 3:
        ks.view(np.uint32)[..., -1] = SU.NAN_PAYLOAD | 0x80000000
        vs.view(np.uint32)[..., -2] = SU.NAN_PAYLOAD
        vs[..., -3] = -np.abs(vs[..., -3])
    return layer


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("fmt", ("e4m3", "e5m2"))
def test_scaled_fp8_single_length_and_ragged(fmt, D):
    """Per-token K and V scale pools stored [N, H, P] / [N, P, H] (one layer each way), fresh pages
    of the same pools: K, V and both scale pools compared whole.  Then lengths 0 / 37 / 512 / 513 /
    1 500 in one ragged call."""
    import fp8_gpu as G
    import scaled_gpu as SG
    import scaled_util as SU
    from kvcompress import compress_paged
    from test_scaled_methods_gpu import _norms, _ragged_expect, _ragged_layers
    for method in ("fix_size_l2", "h2o_l2"):
        kw = SU.KWARGS[method]
        layers = [_plant(l) for l in SU.method_layers(96000 + D, D, fmt)]
        pos = SU.kept_positions(SU.ORACLE_FNS[method], [_norms(l, fmt) for l in layers], **kw)
        with RP.spare(16 + 1):
            pools = [SG.ScaledPool([l], fmt, 16, 96500 + i, G.STORAGES[i % 2],
                                   SG.SCALE_STORAGES[i % 2]) for i, l in enumerate(layers)]
        dsts = [_scaled_dest(p, [256], 96500 + i) for i, p in enumerate(pools)]
        snaps = [p.snapshot() for p in pools]
        lens = compress_paged(method, [p.paged() for p in pools],
                              out=[d.paged_dest() for d in dsts], **kw)
        torch.cuda.synchronize()
        assert lens == [p_.shape[2] for p_ in pos] == [256, 256]
        for li, (pool, d, snap) in enumerate(zip(pools, dsts, snaps)):
            _scaled_expect(pool, d, snap, 0, SU.expected_layer(pos[li], *layers[li]))
            pool.assert_pools(snap, (method, fmt, D, li))
    # ragged, two layers
    layers = [[_plant(s) for s in l] for l in _ragged_layers(97000 + D, D, fmt)]
    kw = SU.KWARGS["fix_size_l2"]
    pos = _ragged_expect("fix_size_l2", kw, layers, fmt)
    new = [min(n, 256) for n in SU.RAGGED_LENS]
    with RP.spare(RP.pages_for(new, 16)):
        pools = [SG.ScaledPool(l, fmt, 16, 97500 + i, G.STORAGES[i % 2], SG.SCALE_STORAGES[i % 2])
                 for i, l in enumerate(layers)]
    dsts = [_scaled_dest(p, new, 97500 + i) for i, p in enumerate(pools)]
    snaps = [p.snapshot() for p in pools]
    lens = compress_paged("fix_size_l2", [p.paged(ragged=True) for p in pools],
                          out=[d.paged_dest() for d in dsts], **kw)
    torch.cuda.synchronize()
    for l, (pool, d, snap) in enumerate(zip(pools, dsts, snaps)):
        assert list(lens[l]) == new == [p_.shape[2] for p_ in pos[l]]
        for b, p_ in enumerate(pos[l]):
            _scaled_expect(pool, d, snap, b, SU.expected_layer(p_, *layers[l][b]))
        pool.assert_pools(snap, ("ragged", fmt, D, l))


def test_scaled_uniform_k_absent_v_and_missing_scale():
    """A uniform-K / absent-V layer: nothing but rows moves.  And destination pools of their own
    without the per-token sides' scale pools are refused before anything is enqueued."""
    import scaled_gpu as SG
    import scaled_util as SU
    from kvcompress import PagedDest, compress_paged
    from test_scaled_methods_gpu import _norms
    fmt, D, kw = "e4m3", 64, SU.KWARGS["fix_size_l2"]
    layer = SU.method_layer(98000, 600, D, fmt)
    with RP.spare(16):
        pool = SG.ScaledPool([layer], fmt, 16, 98100, k_mode="uniform", v_mode="none",
                             uniform=(0.37, None))
    dst = _scaled_dest(pool, [256], 98100)
    pos = SU.kept_positions(SU.ORACLE_FNS["fix_size_l2"], [_norms(layer, fmt, "uniform", 0.37)],
                            **kw)
    snap = pool.snapshot()
    assert compress_paged("fix_size_l2", [pool.paged()], out=[dst.paged_dest()], **kw) == [256]
    torch.cuda.synchronize()
    wk, wv, _, _ = SU.expected_layer(pos[0], *layer)
    _scaled_expect(pool, dst, snap, 0, (wk, wv))
    pool.assert_pools(snap, ("uniform K, no V",))
    with RP.spare(16):
        per_token = SG.ScaledPool([layer], fmt, 16, 98200)
    other = RP.Dest([256], 16, 98201, 2, D, per_token.k.dtype)
    snap, osnap = per_token.snapshot(), other.snapshot()
    with pytest.raises(ValueError, match="need a destination k_scale"):
        compress_paged("fix_size_l2", [per_token.paged()],
                       out=[PagedDest(other.table, other.k, other.v)], **kw)
    torch.cuda.synchronize()
    per_token.assert_pools(snap, ("refused",))
    other.assert_pools(osnap, ("refused",))


# ---- 8: C ABI -------------------------------------------------------------------------------
def _abi_tables(pls, dsts, spec):
    n = len(pls)
    table = np.zeros(n, dtype=N.LAYER_DTYPE)
    pages = np.zeros(n, dtype=N.PAGES_DTYPE)
    pds = np.zeros(n, dtype=N.PAGE_DEST_DTYPE)
    for i, (pl, d) in enumerate(zip(pls, dsts)):
        t = table[i]
        t["k"], t["v"], t["k_out"], t["v_out"] = (x.data_ptr() for x in (pl.k, pl.v, d.k, d.v))
        t["k_stride"] = (0, pl.k.stride(1), pl.k.stride(2))
        t["v_stride"] = (0, pl.v.stride(1), pl.v.stride(2))
        for f, val in spec.items():
            t[f] = val
        pages[i] = (pl.table.data_ptr(), pl.table.stride(0), pl.k.stride(0), pl.v.stride(0),
                    pl.P, pl.k.size(0), 0, 0)
        pds[i] = (d.table.data_ptr(), d.table.stride(0), d.k.stride(0), d.v.stride(0),
                  (d.k.stride(1), d.k.stride(2)), (d.v.stride(1), d.v.stride(2)), d.P, d.k.size(0))
    return table, pages, pds


def test_abi_33_layers_wide_table_and_bad_destination_page_ids():
    """33 layers cross the 32-layer argument chunk; the destination tables are one column wider
    than needed; a destination page id of -1 (layer 0) and one equal to num_pages (layer 32) each
    drop exactly that page's rows and set KVC_DEV_INDEX_RANGE in a caller-owned status word."""
    S, spec = 100, dict(seq_len=100, sink_len=3, tail_start=40, tail_len=45)
    n = 48
    shape = (1, 2, S, 32)
    layers = [(prng.gen_keys(44000 + i, shape, "bf16"), prng.gen_values(44000 + i, shape, "bf16"))
              for i in range(33)]
    pls = [PU.Layer(k, v, 16, 44000 + i) for i, (k, v) in enumerate(layers)]
    dsts = [RP.Dest([n], 8, 44100 + i, 2, 32, torch.bfloat16) for i in range(33)]
    table, pages, pds = _abi_tables(pls, dsts, spec)
    lost = {0: int(dsts[0].table_np[0, 2]), 32: int(dsts[32].table_np[0, 5])}
    dsts[0].table[0, 2] = -1
    dsts[32].table[0, 5] = dsts[32].k.size(0)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = N.Params(dtype=N.KVC_BF16, batch=1, heads=2, head_dim=32, order=0, algo=0,
                 phases=N.PHASE_ALL, external_index=0, device_status=status.data_ptr())
    rc, info = N.plan_repage(p, table, pages, None, None, pds, None)
    assert rc == 0 and all(t["n_out"] == n for t in table)
    ws = torch.full((max(int(info.workspace_bytes), 256),), 0xFF, dtype=torch.uint8, device=DEV)
    snaps, src_snaps = [d.snapshot() for d in dsts], [pl.snapshot() for pl in pls]
    assert N.launch_repage(p, table, pages, None, None, pds, None, ws.data_ptr(),
                           int(info.workspace_bytes), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == N.DEV_INDEX_RANGE
    status.zero_()
    for i, ((k, v), d, snap) in enumerate(zip(layers, dsts, snaps)):
        want = [np.concatenate([x[:, :, :3], x[:, :, 40:85]], axis=2) for x in (k, v)]
        d.expect(snap, *want)
        if i in lost:  # the dropped page keeps its poison
            for back, storage in ((snap[0], d.k_storage), (snap[1], d.v_storage)):
                PU.pool_view(back, storage)[lost[i]].view(torch.uint8).fill_(PU.POISON)
        d.assert_pools(snap, ("abi", i))
        pls[i].assert_pools(src_snaps[i], ("abi source", i))


def test_scaled_17_layers_cross_the_scale_carrying_chunk():
    """17 scale-carrying layers in one launch: the argument chunk of that copy holds 16."""
    import fp8_gpu as G
    import scaled_gpu as SG
    import scaled_util as SU
    from kvcompress import compress_paged
    from test_scaled_methods_gpu import _norms
    fmt, D, kw = "e5m2", 64, SU.KWARGS["fix_size_l2"]
    layers = SU.method_layers(99000, D, fmt, lens=(300,) * 17)
    pos = SU.kept_positions(SU.ORACLE_FNS["fix_size_l2"], [_norms(l, fmt) for l in layers], **kw)
    with RP.spare(16):
        pools = [SG.ScaledPool([l], fmt, 16, 99100 + i, G.STORAGES[i % 2],
                               SG.SCALE_STORAGES[i % 2]) for i, l in enumerate(layers)]
    dsts = [_scaled_dest(p, [256], 99100 + i) for i, p in enumerate(pools)]
    snaps = [p.snapshot() for p in pools]
    assert compress_paged("fix_size_l2", [p.paged() for p in pools],
                          out=[d.paged_dest() for d in dsts], **kw) == [256] * 17
    torch.cuda.synchronize()
    for li, (pool, d, snap) in enumerate(zip(pools, dsts, snaps)):
        _scaled_expect(pool, d, snap, 0, SU.expected_layer(pos[li], *layers[li]))
        pool.assert_pools(snap, ("17 layers", li))


def test_ragged_33_layers_cross_the_argument_chunk():
    """33 ragged layers through destination tables in one launch: the argument chunk holds 32."""
    from kvcompress import compress_paged
    kw = dict(fix_kv_size=48, keep_ratio=0.25, skip_layers=[])
    lens = [100, 37]
    layers_np, pls, dsts = _ragged_setup(45000, lens, 32, "bf16", 16, 33, ("nhpd", "nphd"), 48,
                                         True)
    ref = RU.oracle_per_sequence("fix_size_l2", kw, layers_np)
    snaps = [d.snapshot() for d in dsts]
    got = compress_paged("fix_size_l2", [pl.paged for pl in pls],
                         out=[d.paged_dest() for d in dsts], **kw)
    torch.cuda.synchronize()
    for l in range(33):
        assert list(got[l]) == [48, 37], (l, got[l])
        for b in range(len(lens)):
            rk, rv, kind = ref[l][b]
            rk, rv = layers_np[l][b] if kind == "same" else (rk, rv)
            dsts[l].expect(snaps[l], rk, rv, b)
        dsts[l].assert_pools(snaps[l], ("ragged 33 layers", l))


def test_ragged_scaled_17_layers_cross_the_scale_carrying_chunk():
    """17 ragged scale-carrying layers in one launch: the argument chunk of that copy holds 16.
    (D = 64: the narrowest fp8 row.)"""
    import fp8_gpu as G
    import scaled_gpu as SG
    import scaled_util as SU
    from kvcompress import compress_paged
    from test_scaled_methods_gpu import _ragged_expect
    fmt, D, kw = "e5m2", 64, dict(SU.KWARGS["fix_size_l2"], fix_kv_size=48)
    lens, new = (100, 37), [48, 37]
    layers = [[SU.method_layer(99500 + 100 * l + b, n, D, fmt) for b, n in enumerate(lens)]
              for l in range(17)]
    pos = _ragged_expect("fix_size_l2", kw, layers, fmt)
    with RP.spare(RP.pages_for(new, 16)):
        pools = [SG.ScaledPool(l, fmt, 16, 99600 + i, G.STORAGES[i % 2], SG.SCALE_STORAGES[i % 2])
                 for i, l in enumerate(layers)]
    dsts = [_scaled_dest(p, new, 99600 + i) for i, p in enumerate(pools)]
    snaps = [p.snapshot() for p in pools]
    got = compress_paged("fix_size_l2", [p.paged(ragged=True) for p in pools],
                         out=[d.paged_dest() for d in dsts], **kw)
    torch.cuda.synchronize()
    for l, (pool, d, snap) in enumerate(zip(pools, dsts, snaps)):
        assert list(got[l]) == new == [p_.shape[2] for p_ in pos[l]]
        for b, p_ in enumerate(pos[l]):
            _scaled_expect(pool, d, snap, b, SU.expected_layer(p_, *layers[l][b]))
        pool.assert_pools(snap, ("ragged 17 layers", l))


# ---- 8 (phases), 9, 10, 11: the C ABI's promises on the new copy kernels -----------------------
def _fields(s):
    """kvc_layer_t segment fields of a phase_tables spec."""
    return dict(seq_len=s["S"], zone_start=s["zone_start"], zone_len=s["zone_len"],
                n_select=s["n_select"], sink_len=s["sink"], tail_start=s["tail_start"],
                tail_len=s["tail_len"], score_mode=s["score_mode"], pool_kernel=s["pool"])


class _Repage:
    """One planned kvc_launch_repage: params with a caller-owned status word, a 0xFF workspace."""

    def __init__(self, dtype, B, H, D, table, pages, pds, ragged=None, scales=None, dscales=None,
                 external=0):
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.p = N.Params(dtype=dtype, batch=B, heads=H, head_dim=D, order=0, algo=0,
                          phases=N.PHASE_GATHER if external else N.PHASE_ALL,
                          external_index=external, device_status=self.status.data_ptr())
        self.args = (table, pages, ragged, scales, pds, dscales)
        rc, self.info = N.plan_repage(self.p, *self.args)
        assert rc == 0, rc
        self.ws = torch.full((max(int(self.info.workspace_bytes), 256),), 0xFF, dtype=torch.uint8,
                             device=DEV)

    def indices(self, idx, B, H):
        """Caller-written index rows (idx [B, H, n]) of a one-layer table."""
        rows = np.full((int(self.info.rows), int(self.info.index_row_stride)), -1, dtype=np.int32)
        rows[:B * H, :idx.shape[-1]] = idx.reshape(B * H, -1)
        off = int(self.info.index_offset)
        self.ws[off:off + rows.size * 4].view(torch.int32).copy_(
            torch.from_numpy(rows.reshape(-1)))

    def run(self, phases=None, sync=True, status=0):
        if phases is not None:
            self.p.phases = phases
        rc = N.launch_repage(self.p, *self.args, self.ws.data_ptr(),
                             int(self.info.workspace_bytes),
                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        if sync:
            torch.cuda.synchronize()
            assert int(self.status.item()) == status
            self.status.zero_()


def test_phases_launched_one_at_a_time_equal_one_launch():
    """8: SCORE, SELECT and GATHER as three kvc_launch_repage calls on a 0xFF-filled workspace
    leave the bytes of one launch, which are the CPU expectation's."""
    import phase_tables as PT
    s = PT.spec(700, zone_start=30, zone_len=500, n_select=260, sink=4, tail_start=545,
                tail_len=150, variant="few")
    B, H, D = 2, 3, 64
    (kn, vn), = PT.gen_layers([s], B, H, D, "bf16")
    wk, wv, _ = PT.expected_layer(kn, vn, s, PT.ASC, PT.SORT)
    backs = []
    for steps in ((N.PHASE_ALL,), (N.PHASE_SCORE, N.PHASE_SELECT, N.PHASE_GATHER)):
        pl = PU.Layer(kn, vn, 16, 45000)
        dst = RP.Dest([PT.n_out(s)] * B, 16, 45001, H, D, torch.bfloat16)
        snap, src = dst.snapshot(), pl.snapshot()
        r = _Repage(N.KVC_BF16, B, H, D, *_abi_tables([pl], [dst], _fields(s)))
        for ph in steps:
            r.run(ph)
        dst.expect(snap, wk, wv)
        dst.assert_pools(snap, ("phases", steps))
        pl.assert_pools(src, ("phases source", steps))
        backs.append((dst.kb, dst.vb))
    assert torch.equal(PU.ints(backs[0][0]), PU.ints(backs[1][0]))
    assert torch.equal(PU.ints(backs[0][1]), PU.ints(backs[1][1]))


@pytest.mark.parametrize("D", (32, 80, 256))
@pytest.mark.parametrize("dtype", ("bf16", "fp16", "fp32"))
def test_nan_rewrite_on_gather_repage_kernel(dtype, D):
    """9: test_nan_payload_gpu's pattern table and spec (every NaN pattern of the dtype in both
    halves of a word, in K and V) through gather_repage_kernel with caller-written indices: the
    gathered segment is rewritten as torch.gather does, sink and tail rows are copied; whole
    destination pools compared, the source unchanged."""
    import test_nan_payload_gpu as NP
    K, V = NP._copy_inputs(dtype, D)
    idx = NP._picks(90 + D)
    wk, wv = NP._expected(dtype, D, idx[0])
    pl = PU.Layer(K, V, 16, 600 + D)
    dst = RP.Dest([NP.N_OUT] * NP.B, 16, 601 + D, NP.H, D, NP.TDT[dtype])
    snap, src = dst.snapshot(), pl.snapshot()
    r = _Repage(NP.DT[dtype], NP.B, NP.H, D, *_abi_tables([pl], [dst], _fields(NP.SPEC)),
                external=1)
    r.indices(idx[0], NP.B, NP.H)
    r.run()
    dst.expect(snap, wk, wv)
    dst.assert_pools(snap, ("nan", dtype, D))
    pl.assert_pools(src, ("nan source", dtype, D))


def test_destination_offsets_past_4_gib():
    """10: the one destination page that receives rows lies more than 4 GiB above its pool's
    base (modelled on test_paged_gpu's test_offsets_past_4_gib)."""
    from kvcompress import PagedDest, compress_paged
    from oracle import oracle
    B, H, S, P, D = 1, 2, 300, 128, 64
    page_elems = H * P * D
    gap = (1 << 31) // 2 + page_elems           # elements: 2 GiB + one page of bf16 per step
    kn, vn = prng.gen_keys(47100, (B, H, S, D), "bf16"), prng.gen_values(47100, (B, H, S, D), "bf16")
    pl = PU.Layer(kn, vn, 16, 47100)
    flat = torch.empty(2 * gap + page_elems, dtype=torch.bfloat16, device=DEV)
    vflat = torch.empty(3 * page_elems, dtype=torch.bfloat16, device=DEV)
    k_dst = flat.as_strided((3, H, P, D), (gap, P * D, D, 1))
    v_dst = vflat.as_strided((3, H, P, D), (page_elems, D, H * D, 1))
    assert 2 * gap * 2 > 1 << 32
    for pool in (k_dst, v_dst):
        pool.fill_(1.5)
    table = torch.tensor([[2, 0, 1]], dtype=torch.int32, device=DEV)
    snap, src = (k_dst.clone(), v_dst.clone()), pl.snapshot()
    kw = dict(fix_kv_size=100, keep_ratio=0.25, skip_layers=[])
    (rk, rv, _), = oracle.METHODS["fix_size_l2"]([(kn, vn)], **kw)
    lens = compress_paged("fix_size_l2", [pl.paged], out=[PagedDest(table, k_dst, v_dst)], **kw)
    torch.cuda.synchronize()
    assert lens == [100]
    PU.write_rows(snap[0], table, to_dev(rk, DEV))
    PU.write_rows(snap[1], table, to_dev(rv, DEV))
    assert torch.equal(PU.ints(k_dst), PU.ints(snap[0]))
    assert torch.equal(PU.ints(v_dst), PU.ints(snap[1]))
    pl.assert_pools(src, ("4 GiB source",))


def _set_table(dst, rows):
    """Rewrite the device table of a Dest to the page rows `rows` (one int64 array per sequence)."""
    full = np.full(tuple(dst.table.shape), -1, dtype=np.int32)
    for b, r in enumerate(rows):
        full[b, :len(r)] = r
    dst.table.copy_(torch.from_numpy(full).to(DEV))
    dst.rows = list(rows)


def test_captured_single_length_launch_follows_the_destination_table():
    """11a: kvc_launch_repage captured after a warm-up; the destination table is rewritten to other
    fresh pages before each replay, and each replay lands where the table then points."""
    import phase_tables as PT
    s = PT.spec(700, zone_start=30, zone_len=500, n_select=260, sink=4, tail_start=545,
                tail_len=150)
    B, H, D = 2, 3, 64
    (kn, vn), = PT.gen_layers([s], B, H, D, "bf16")
    wk, wv, _ = PT.expected_layer(kn, vn, s, PT.ASC, PT.SORT)
    pl = PU.Layer(kn, vn, 16, 45100)
    n = PT.n_out(s)
    big = RP.Dest([n] * (3 * B), 16, 45101, H, D, torch.bfloat16)   # three sets of pages
    sets = [big.rows[i * B:(i + 1) * B] for i in range(3)]
    dst = RP.Dest([n] * B, 16, 45101, pool=(big.kb, big.vb, big.k, big.v, big.k_storage,
                                             big.v_storage), used=0)
    r = _Repage(N.KVC_BF16, B, H, D, *_abi_tables([pl], [dst], _fields(s)))
    src = pl.snapshot()

    def check(rows, go, what):
        _set_table(dst, rows)
        snap = dst.snapshot()
        go()
        torch.cuda.synchronize()
        assert int(r.status.item()) == 0
        dst.expect(snap, wk, wv)
        dst.assert_pools(snap, ("graph", what))
        pl.assert_pools(src, ("graph source", what))

    check(sets[0], lambda: r.run(sync=False), "warm-up")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r.run(sync=False)
    check(sets[1], g.replay, "replay 1")
    check(sets[2], g.replay, "replay 2")


def test_captured_ragged_launch_follows_tables_and_records():
    """11b: the ragged launch captured; before each replay the pools are refilled with other
    sequences, the device records rewritten to other lengths inside the planned envelope, and the
    destination table rewritten to other fresh pages.  Passed-through sequences are copied."""
    from kvcompress import _engine as E
    from kvcompress import paged
    from kvcompress.methods import get_compress_fn
    kw = dict(fix_kv_size=512, keep_ratio=0.25, skip_layers=[])
    room, first, second = [1500, 1500, 600], [1500, 900, 37], [700, 1500, 600]
    L, H, D, B = 2, 2, 64, 3
    _, pls = RU.build(5600, room, H, D, "bf16", 16, L)
    bigs = [RP.Dest([512] * (3 * B), 16, 45200 + l, H, D, torch.bfloat16) for l in range(L)]
    dsts = [RP.Dest([512] * B, 16, 0, pool=(g.kb, g.vb, g.k, g.v, g.k_storage, g.v_storage))
            for g in bigs]
    geo = [(H, D, torch.bfloat16, pl.k.device) for pl in pls]

    def records(lens):
        rec, _, new = paged.plan_ragged(get_compress_fn("fix_size_l2"), [lens] * L, geo, kw,
                                        unordered=set(range(L)))
        return np.ascontiguousarray(rec), new

    host, _ = records(first)
    dev = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(DEV)
    spec = dict()
    table, pages, pds = _abi_tables(pls, dsts, spec)
    ragged = np.zeros(L, dtype=N.RAGGED_DTYPE)
    for l in range(L):
        ragged[l] = (host[l].ctypes.data, dev.data_ptr() + l * B * N.SEQ_DTYPE.itemsize)
    r = _Repage(N.KVC_BF16, B, H, D, table, pages, pds, ragged=ragged)
    assert E is not None

    def run(lens, seed, go, which):
        layers_np = [RU.gen_sequences(seed + 1000 * l, lens, H, D, "bf16") for l in range(L)]
        for pl, seqs in zip(pls, layers_np):
            pl.fill(seqs)
        rec2, new = records(lens)
        dev.copy_(torch.from_numpy(rec2.view(np.uint8).reshape(-1)))
        for g, d in zip(bigs, dsts):
            _set_table(d, g.rows[which * B:(which + 1) * B])
        snaps = [d.snapshot() for d in dsts]
        srcs = [pl.snapshot() for pl in pls]
        go()
        torch.cuda.synchronize()
        assert int(r.status.item()) == 0
        ref = RU.oracle_per_sequence("fix_size_l2", kw, layers_np)
        for l, (d, snap) in enumerate(zip(dsts, snaps)):
            for b in range(B):
                rk, rv, kind = ref[l][b]
                rk, rv = layers_np[l][b] if kind == "same" else (rk, rv)
                assert new[l][b] == rk.shape[2]
                d.expect(snap, rk, rv, b)
            d.assert_pools(snap, ("ragged graph", lens, l))
            pls[l].assert_pools(srcs[l], ("ragged graph source", lens, l))

    run(first, 5610, lambda: r.run(sync=False), 0)  # the warm-up
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r.run(sync=False)
    run(first, 5620, g.replay, 1)
    run(second, 5630, g.replay, 2)


@pytest.mark.parametrize("bad", ("minus one", "num_pages"))
def test_bad_destination_page_id_drops_rows_and_scale_words(bad):
    """8: a scale-carrying layer whose destination table names page -1 / page num_pages for output
    rows [16, 32): exactly those rows' K, V and scale stores are dropped (K, V and both scale
    pools compared whole), KVC_DEV_INDEX_RANGE is set, every other row is correct."""
    import scaled_gpu as SG
    import scaled_util as SU
    fmt, D, S = "e4m3", 64, 100
    layer = SU.method_layer(99500, S, D, fmt)
    with RP.spare(3):
        pool = SG.ScaledPool([layer], fmt, 16, 99600)
    dst = _scaled_dest(pool, [48], 99600)
    spec = dict(seq_len=S, sink_len=3, tail_start=40, tail_len=45)
    table, pages, pds = _abi_tables([pool], [dst], spec)
    z = pool.scales_row()
    lost = int(dst.rows[0][1])
    dst.table[0, 1] = -1 if bad == "minus one" else pool.k.size(0)
    r = _Repage(N.KVC_F8E4M3, 1, 2, D, table, pages, pds, scales=z, dscales=z.copy())
    snap = pool.snapshot()
    r.run(status=N.DEV_INDEX_RANGE)
    pos = np.broadcast_to(np.concatenate([np.arange(3), np.arange(40, 85)]), (1, 2, 48))
    _scaled_expect(pool, dst, snap, 0, SU.expected_layer(pos, *layer))
    for back, storage in ((snap[0], pool.storages[0]), (snap[1], pool.storages[1])):
        PU.pool_view(back, storage)[lost].fill_(PU.POISON)   # (uint8 backings)
    for side in range(2):
        SG.scale_view(snap[2 + side], pool.scale_storages[side], 2, 16)[lost].fill_(0x5A5A5A5A)
    pool.assert_pools(snap, ("bad scaled id", bad))
