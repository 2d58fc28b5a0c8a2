"""SCORE of fp8 keys alone through the C ABI (KVC_PHASE_SCORE): the decode of every bit pattern at
every byte lane, torch.norm's accumulator order on the bf16 upcast, and the bf16 norm region.

Keys [16, 2, S, D] from fp8_util.score_keys: the first 16 (b, h) rows are the 16 byte lanes of a
16-byte chunk.  Zone token t < 256 of row r < 16 carries bit pattern t at every element d with
d % 16 == r and ZERO elsewhere, so the row's norm is the pattern's own -- |x| * sqrt(D / 16), which
bf16 tells apart for every magnitude of the format (test_fp8_cpu shows that a wrong decode of any
pattern at any lane would move a norm byte; a sign cannot show in a norm).  Rows 16 .. 31 carry the
same patterns over a background of quantised normal values: the decode inside the accumulator
order with every lane busy.  NaN patterns make their rows NaN, e5m2's +-inf an inf norm.  Zone
token 256 -- the 1-token tile -- holds the further rows: all zero, all subnormal, all maximal, one
NaN, one inf (e5m2), and the summation-order probes of fp8_util.order_rows.  The norm region is
compared byte for byte with torch.norm(K.to(bfloat16), dim=-1) on the CPU and with oracle.norms,
in norm and snapkv mode (tile maxima included), on a 0xFF-filled workspace: dense, through windows
of a static cache and of a fused QKV buffer, paged at P = 1 / 16 / 64 in both pool storages, and
ragged.
"""
import numpy as np
import pytest
import torch

import fp8_gpu as G
import fp8_util as F
import phase_tables as PT
from kvcompress import _native as N
from oracle import oracle

pytestmark = pytest.mark.gpu

B, H, S = F.SCORE_B, F.SCORE_H, F.SCORE_S
ZONE_START, ZONE_LEN = F.SCORE_ZONE_START, F.SCORE_ZONE_LEN
TILE = 64
score_keys = F.score_keys


def expected_norms(k8, fmt):
    """[B * H, ZONE_LEN] bf16 bits: oracle.norms and torch.norm on the CPU upcast, which agree."""
    zone = k8[:, :, ZONE_START:ZONE_START + ZONE_LEN]
    want = oracle.norms(F.to_bf16_bits(zone, fmt))
    t = torch.from_numpy(np.ascontiguousarray(zone)).view(F.torch_dtype(fmt)).to(torch.bfloat16)
    ref = torch.norm(t, p=2, dim=-1).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(ref, want)
    return want.reshape(-1, ZONE_LEN)


def tile_maxima(want):
    nt = -(-ZONE_LEN // TILE)
    pad = np.zeros((want.shape[0], nt * TILE), dtype=np.uint32)
    pad[:, :want.shape[1]] = want
    return pad.reshape(want.shape[0], nt, TILE).max(axis=2)


def _spec(mode, zone_start=ZONE_START, zone_len=ZONE_LEN, seq=S):
    k = min(40, zone_len - 1)
    return dict(PT.spec(seq, zone_start=zone_start, zone_len=zone_len, n_select=max(k, 0),
                        sink=min(3, zone_start), tail_start=zone_start + zone_len, tail_len=0,
                        score_mode=mode, pool=5 if mode == PT.SNAPKV else 0), S=seq)


def _check(L, want, ctx, mode):
    L.run(N.PHASE_SCORE)
    norms, tmax = L.regions()
    assert np.array_equal(norms[:, :ZONE_LEN], want), ctx
    if mode == PT.SNAPKV:
        assert np.array_equal(tmax[:, :-(-ZONE_LEN // TILE)], tile_maxima(want)), ctx + ("tmax",)


def _modes():
    return ((PT.NORM, PT.ASC, PT.SORT), (PT.SNAPKV, PT.DESC, PT.TOPK))


@pytest.mark.parametrize("D", (64, 128, 256))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_score_decodes_every_pattern_at_every_lane(fmt, D):
    k8 = score_keys(fmt, D)
    want = expected_norms(k8, fmt)
    nan_rows = ((want & 0x7FFF) > 0x7F80)
    assert nan_rows[:, :256].sum() == B * H * len(F.NAN_CODES[fmt])  # only the NaN patterns' rows
    assert (want == 0x7F80).sum() >= (B * H * 2 + 2 if fmt == "e5m2" else 0)
    v8 = F.gen_values(61500 + D, (B, H, S, D), fmt)
    k, v = G.dev8(k8, fmt), G.dev8(v8, fmt)
    kb, vb = k.clone(), v.clone()
    n = 43
    outs = [torch.zeros((B, H, n, D), dtype=torch.uint8, device=G.DEV) for _ in range(2)]
    # strided sources: a window of a static cache [B, H, S + 11, D] and the K third of a fused
    # [B, S, 3, H, D] buffer
    cache = torch.zeros((B, H, S + 11, D), dtype=torch.uint8, device=G.DEV)
    cache[:, :, 6:6 + S] = G.as_u8(k)
    fused = torch.zeros((B, S, 3, H, D), dtype=torch.uint8, device=G.DEV)
    fused[:, :, 1] = G.as_u8(k).permute(0, 2, 1, 3)
    t8 = F.torch_dtype(fmt)
    sources = {"dense": k, "cache window": cache[:, :, 6:6 + S].view(t8),
               "fused third": fused[:, :, 1].permute(0, 2, 1, 3).view(t8)}
    for mode, order, algo in _modes():
        for name, src in sources.items():
            assert name == "dense" or not src.is_contiguous()
            table = np.array([G.layer_row(_spec(mode), S, src, v, outs[0], outs[1])],
                             dtype=N.LAYER_DTYPE)
            L = G.Launch(G.KVC[fmt], B, H, D, order, algo, table, flags=N.FLAG_SPLIT_SELECT_GATHER)
            _check(L, want, (fmt, D, mode, name), mode)
        for P in (1, 16, 64):
            for st in G.STORAGES:
                pool = G.Pool((k8, v8), fmt, P, 62000 + P, st)
                snap = pool.snapshot()
                table = np.array([G.layer_row(_spec(mode), S, ko=outs[0], vo=outs[1], pool=pool)],
                                 dtype=N.LAYER_DTYPE)
                L = G.Launch(G.KVC[fmt], B, H, D, order, algo, table, pages=G.pages_row(pool))
                _check(L, want, (fmt, D, mode, "paged", P, st), mode)
                pool.assert_pools(snap, (fmt, D, P, st))
    assert not outs[0].any() and not outs[1].any()  # SCORE alone writes no output
    assert torch.equal(G.as_u8(k), G.as_u8(kb)) and torch.equal(G.as_u8(v), G.as_u8(vb))


@pytest.mark.parametrize("D", (64, 128, 256))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_ragged_score(fmt, D):
    """Sequences of 0 / 37 / 257 rows in one ragged launch: sequence b is the leading rows of the
    dense zone of batch row b, so its norm row is the leading part of the dense expectation."""
    k8 = score_keys(fmt, D)
    want = expected_norms(k8, fmt).reshape(B, H, ZONE_LEN)
    v8 = F.gen_values(61500 + D, (B, H, S, D), fmt)
    lens = (0, 37, 257)
    z = slice(ZONE_START, ZONE_START + ZONE_LEN)
    seqs = [(k8[b:b + 1, :, z][:, :, :n], v8[b:b + 1, :, z][:, :, :n])
            for b, n in enumerate(lens)]
    for mode, order, algo in _modes():
        for P, st in ((1, G.STORAGES[0]), (16, G.STORAGES[1]), (64, G.STORAGES[0])):
            pool = G.Pool(seqs, fmt, P, 63000 + P, st)
            snap = pool.snapshot()
            specs = [dict(PT.spec(0), S=0) if n == 0 else _spec(mode, 0, n, n) for n in lens]
            host, dev = G.seq_records(specs)
            ragged = np.zeros(1, dtype=N.RAGGED_DTYPE)
            ragged[0] = (host.ctypes.data, dev.data_ptr())
            table = np.array([G.layer_row(_spec(mode, 0, 257, 257), 257, pool=pool)],
                             dtype=N.LAYER_DTYPE)
            L = G.Launch(G.KVC[fmt], len(lens), H, D, order, algo, table,
                         pages=G.pages_row(pool, in_place=1), ragged=ragged)
            L.run(N.PHASE_SCORE)
            norms, tmax = L.regions()
            for b, n in enumerate(lens):
                ctx = (fmt, D, mode, P, st, n)
                got = norms[b * H:(b + 1) * H, :n]
                assert np.array_equal(got, want[b, :, :n]), ctx
                if mode == PT.SNAPKV and n:
                    nt = -(-n // TILE)
                    pad = np.zeros((H, nt * TILE), dtype=np.uint32)
                    pad[:, :n] = want[b, :, :n]
                    assert np.array_equal(tmax[b * H:(b + 1) * H, :nt],
                                          pad.reshape(H, nt, TILE).max(axis=2)), ctx + ("tmax",)
            pool.assert_pools(snap, (fmt, D, P, st))
