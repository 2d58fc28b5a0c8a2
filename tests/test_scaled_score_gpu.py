"""SCORE of per-token-scaled fp8 keys alone through the C ABI (kvc_launch_scaled with
KVC_PHASE_SCORE): the norm region, byte for byte, is the contract's

    bf16( torch.norm(K8.to(float32), dim=-1) * |s| )

(scaled_util.stored_norms; test_scaled_cpu pins it against that torch expression).  Keys
[2, 2, 130, D] -- two full 64-token tiles and a 2-token one -- with scales that are powers of two,
ordinary values whose product needs rounding, +-0, negative, +-inf, NaN, and values that make the
product an fp32 denormal and a bf16 denormal (scaled_util.score_case): a device that flushed a
denormal product would fail here.  D = 64 / 128 / 256, both formats, P = 1 / 16 / 64, the K pool
stored [N, H, P, D] and [N, P, H, D], the scale pool [N, H, P] and [N, P, H] (strided, padded),
shuffled page ids, norm and snapkv mode (tile maxima included), on a 0xFF-filled workspace; a
uniform scale; a layer without K scales (its V scales are never read); the single-length and the
ragged kernel (lengths 0 / 37 / 130).  SCORE alone writes no pool byte."""
import numpy as np
import pytest
import torch

import fp8_gpu as G
import fp8_util as F
import phase_tables as PT
import scaled_gpu as SG
import scaled_util as SU
from kvcompress import _native as N

pytestmark = pytest.mark.gpu

B, H, S = SU.SCORE_B, SU.SCORE_H, SU.SCORE_S
TILE = 64
MODES = ((PT.NORM, PT.ASC, PT.SORT), (PT.SNAPKV, PT.DESC, PT.TOPK))
GEOMETRIES = [(P, st, sst) for P in (1, 16, 64) for st in G.STORAGES for sst in SG.SCALE_STORAGES]


def _spec(mode, n=S):
    return dict(PT.spec(n, zone_start=0, zone_len=n, n_select=min(40, n - 1), sink=0, tail_start=n,
                        tail_len=0, score_mode=mode, pool=5 if mode == PT.SNAPKV else 0), S=n)


def _tile_maxima(want):
    n = want.shape[-1]
    nt = -(-n // TILE)
    pad = np.zeros((want.shape[0], nt * TILE), dtype=np.uint32)
    pad[:, :n] = want
    return pad.reshape(want.shape[0], nt, TILE).max(axis=2)


def _seqs(k8, v8, s, vs):
    return [(k8[b:b + 1], v8[b:b + 1], s[b:b + 1], vs[b:b + 1]) for b in range(k8.shape[0])]


def _score(pool, fmt, D, mode, order, algo):
    table = np.array([G.layer_row(_spec(mode), S, pool=pool)], dtype=N.LAYER_DTYPE)
    L = SG.Launch(G.KVC[fmt], B, H, D, order, algo, table, G.pages_row(pool, in_place=1),
                  pool.scales_row())
    L.run(N.PHASE_SCORE)
    return L.regions()


def _check(pool, fmt, D, want, ctx):
    snap = pool.snapshot()
    for mode, order, algo in MODES:
        norms, tmax = _score(pool, fmt, D, mode, order, algo)
        assert np.array_equal(norms[:, :S], want), ctx + (mode,)
        if mode == PT.SNAPKV:
            assert np.array_equal(tmax[:, :-(-S // TILE)], _tile_maxima(want)), ctx + ("tmax",)
    pool.assert_pools(snap, ctx)


@pytest.mark.parametrize("D", (64, 128, 256))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_per_token_scales(fmt, D):
    k8, s = SU.score_case(fmt, D)
    v8 = F.gen_values(83000 + D, (B, H, S, D), fmt)
    vs = np.full(s.shape, 7.5, dtype=np.float32)  # never read: would move every norm
    want = SU.stored_norms(k8, s, fmt).reshape(B * H, S)
    assert (want != F.norms_bf16(k8, fmt).reshape(B * H, S)).mean() > 0.9
    for P, st, sst in GEOMETRIES:
        pool = SG.ScaledPool(_seqs(k8, v8, s, vs), fmt, P, 84000 + P, st, sst)
        _check(pool, fmt, D, want, (fmt, D, P, st, sst))


@pytest.mark.parametrize("D", (64, 128, 256))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_uniform_and_absent_k_scales(fmt, D):
    k8, s = SU.score_case(fmt, D)
    v8 = F.gen_values(83000 + D, (B, H, S, D), fmt)
    for u in SU.UNIFORM_SCALES:
        want = SU.stored_norms(k8, np.float32(u), fmt).reshape(B * H, S)
        for v_mode in ("pool", "uniform", "none"):
            pool = SG.ScaledPool(_seqs(k8, v8, s, s), fmt, 16, 85000, k_mode="uniform",
                                 v_mode=v_mode, uniform=(u, 3.0))
            _check(pool, fmt, D, want, (fmt, D, "uniform", u, v_mode))
    # no K scale: the unscaled fp8 norms, whatever the V scales are
    want = F.norms_bf16(k8, fmt).reshape(B * H, S)
    pool = SG.ScaledPool(_seqs(k8, v8, s, s), fmt, 16, 85001, G.STORAGES[1], SG.SCALE_STORAGES[1],
                         k_mode="none")
    _check(pool, fmt, D, want, (fmt, D, "no K scale"))


@pytest.mark.parametrize("D", (64, 128, 256))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_ragged_score(fmt, D):
    """Sequences of 0 / 37 / 130 rows in one ragged launch: sequence b is the leading rows of
    batch row b % 2, so its norm row is the leading part of that row's expectation."""
    k8, s = SU.score_case(fmt, D)
    v8 = F.gen_values(83000 + D, (B, H, S, D), fmt)
    want = SU.stored_norms(k8, s, fmt)
    lens = (0, 37, 130)
    seqs = [(k8[b % B:b % B + 1, :, :n], v8[b % B:b % B + 1, :, :n], s[b % B:b % B + 1, :, :n],
             s[b % B:b % B + 1, :, :n]) for b, n in enumerate(lens)]
    for mode, order, algo in MODES:
        for P, st, sst in ((1, G.STORAGES[0], SG.SCALE_STORAGES[1]),
                           (16, G.STORAGES[1], SG.SCALE_STORAGES[0]),
                           (64, G.STORAGES[0], SG.SCALE_STORAGES[0])):
            pool = SG.ScaledPool(seqs, fmt, P, 86000 + P, st, sst)
            snap = pool.snapshot()
            specs = [dict(PT.spec(0), S=0) if n == 0 else _spec(mode, n) for n in lens]
            host, dev = G.seq_records(specs)
            ragged = np.zeros(1, dtype=N.RAGGED_DTYPE)
            ragged[0] = (host.ctypes.data, dev.data_ptr())
            table = np.array([G.layer_row(_spec(mode), S, pool=pool)], dtype=N.LAYER_DTYPE)
            L = SG.Launch(G.KVC[fmt], len(lens), H, D, order, algo, table,
                          G.pages_row(pool, in_place=1), pool.scales_row(), ragged=ragged)
            L.run(N.PHASE_SCORE)
            norms, tmax = L.regions()
            for b, n in enumerate(lens):
                ctx = (fmt, D, mode, P, st, sst, n)
                w = want[b % B, :, :n]
                assert np.array_equal(norms[b * H:(b + 1) * H, :n], w), ctx
                if mode == PT.SNAPKV and n:
                    assert np.array_equal(tmax[b * H:(b + 1) * H, :-(-n // TILE)],
                                          _tile_maxima(w)), ctx + ("tmax",)
            pool.assert_pools(snap, (fmt, D, P, st, sst))
