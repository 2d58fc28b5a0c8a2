"""SCORE of paged keys on every row width and page size (score_paged_kernel, csrc/kvc_paged.h).

score_paged_tile is a hand-kept copy of score_tile (csrc/kvc_score.h) from `float acc[8]` on, with
every staged token's row address taken through the block table.  Here every chunk count of it -- the
seven chunk counts NC = 4, 8, 10, 16, 20, 32, 64 of strided_layouts.WIDTHS_A, plus bf16 D256 and
fp32 D128, so that NC = 32 runs in all three dtypes -- is launched with KVC_PHASE_SCORE alone on
a 0xFF-filled workspace, at page sizes below, at and above the 64-token tile, and its norm rows
(and snapkv tile maxima) are compared byte for byte with the dense kernel's on the dense tensor
the table describes and with oracle.norms.  Pools: tests/paged_util.py (shuffled table, K stored
[N, H, P, D], V [N, P, H, D], table wider than needed).  Zone [37, 298): four full tiles and one
of 5 tokens, starting in the middle of a page for every P > 1.
"""
import numpy as np
import pytest
import torch

import paged_util as PU
import phase_tables as PT
import prng
import strided_layouts as SL
from gpu_util import to_dev
from kvcompress import _native as N
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = PU.DEV
WIDTHS = SL.WIDTHS_A + ((256, "bf16"), (128, "fp32"))
PAGE_SIZES = (1, 4, 32, 64, 256)
VARIANTS = ("special", "normal")
B, H, S = 2, 3, 330
ZONE_START, ZONE_LEN = 37, 261
KVC_DT = {"bf16": N.KVC_BF16, "fp16": N.KVC_F16, "fp32": N.KVC_F32}
TILE = 64


def test_the_sweep_reaches_every_instance():
    nc = sorted({D * (4 if dt == "fp32" else 2) // 16 for D, dt in WIDTHS})
    assert nc == [4, 8, 10, 16, 20, 32, 64]
    nc32 = {dt for D, dt in WIDTHS if D * (4 if dt == "fp32" else 2) // 16 == 32}
    assert nc32 == {"bf16", "fp16", "fp32"}
    assert -(-ZONE_LEN // TILE) == 5 and ZONE_LEN % TILE == 5
    assert all(ZONE_START % P for P in PAGE_SIZES if P > 1)


def _spec(mode):
    return PT.spec(S, zone_start=ZONE_START, zone_len=ZONE_LEN, n_select=40, sink=3,
                   tail_start=300, tail_len=30, score_mode=mode, pool=5 if mode == PT.SNAPKV else 0)


def _score(dt, D, s, k, v, pl):
    """One KVC_PHASE_SCORE launch of layer spec `s` on dense k / v (pl None) or on the pools of
    `pl`; returns (norm rows [B * H, zone_len * esz] bytes, tile-maxima region bytes)."""
    esz = 4 if dt == "fp32" else 2
    tdt = (k if pl is None else pl.k).dtype
    outs = tuple(torch.zeros((B, H, PT.n_out(s), D), dtype=tdt, device=DEV) for _ in range(2))
    table = np.zeros(1, dtype=N.LAYER_DTYPE)
    t = table[0]
    pages = None
    if pl is None:
        t["k"], t["v"] = k.data_ptr(), v.data_ptr()
        t["k_stride"], t["v_stride"] = k.stride()[:3], v.stride()[:3]
    else:
        t["k"], t["v"] = pl.k.data_ptr(), pl.v.data_ptr()
        t["k_stride"] = (0,) + tuple(pl.k.stride()[1:3])
        t["v_stride"] = (0,) + tuple(pl.v.stride()[1:3])
        pages = np.zeros(1, dtype=N.PAGES_DTYPE)
        pages[0] = (pl.table.data_ptr(), pl.table.stride(0), pl.k.stride(0), pl.v.stride(0), pl.P,
                    pl.k.size(0), 0, 0)
    t["k_out"], t["v_out"] = outs[0].data_ptr(), outs[1].data_ptr()
    t["seq_len"], t["zone_start"], t["zone_len"] = S, s["zone_start"], s["zone_len"]
    t["n_select"], t["sink_len"] = s["n_select"], s["sink"]
    t["tail_start"], t["tail_len"] = s["tail_start"], s["tail_len"]
    t["score_mode"], t["pool_kernel"] = s["score_mode"], s["pool"]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    order, algo = (PT.DESC, PT.TOPK) if s["score_mode"] == PT.SNAPKV else (PT.ASC, PT.SORT)
    p = N.Params(dtype=KVC_DT[dt], batch=B, heads=H, head_dim=D, order=order, algo=algo,
                 phases=N.PHASE_ALL, external_index=0, flags=N.FLAG_SPLIT_SELECT_GATHER,
                 device_status=status.data_ptr())
    rc, info = N.plan_paged(p, table, pages, None)
    assert rc == 0, rc
    ws = torch.full((max(int(info.workspace_bytes), 256),), PT.POISON, dtype=torch.uint8,
                    device=DEV)
    p.phases = N.PHASE_SCORE
    rc = N.launch_paged(p, table, pages, None, ws.data_ptr(), int(info.workspace_bytes),
                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert not outs[0].any() and not outs[1].any()  # SCORE alone writes no output
    rows, ns, istr = int(info.rows), int(info.norm_row_stride), int(info.index_row_stride)
    assert rows == B * H and ns >= ZONE_LEN
    w = ws.cpu().numpy()
    norms = w[info.norm_offset:info.norm_offset + rows * ns * esz].reshape(rows, ns * esz)
    toff = (info.index_offset + rows * istr * 4 + 255) // 256 * 256  # csrc/kvc.hip tmax_offset
    tmax = w[toff:toff + rows * (ns // TILE) * 4]
    return norms[:, :ZONE_LEN * esz].copy(), tmax.copy(), (rows, ns, istr,
                                                           int(info.workspace_bytes))


def _tile_maxima(want, dt):
    """The snapkv tile maxima of oracle norms [B, H, zone_len]: per 64-token tile the largest
    stored norm taken as its unsigned bit pattern (norms are >= 0 or NaN)."""
    bits = np.ascontiguousarray(want).view(np.uint32 if dt == "fp32" else np.uint16)
    bits = bits.reshape(B * H, ZONE_LEN).astype(np.uint32)
    nt = -(-ZONE_LEN // TILE)
    pad = np.zeros((B * H, nt * TILE), dtype=np.uint32)
    pad[:, :ZONE_LEN] = bits
    return pad.reshape(B * H, nt, TILE).max(axis=2)


@pytest.mark.parametrize("D, dt", WIDTHS, ids=[f"{dt}-D{D}" for D, dt in WIDTHS])
def test_paged_score_equals_dense_score_and_oracle(D, dt):
    esz = 4 if dt == "fp32" else 2
    for vi, variant in enumerate(VARIANTS):
        seed = 49000 + 10 * D + vi
        kn = prng.gen_keys(seed, (B, H, S, D), dt, variant)
        vn = prng.gen_values(seed, (B, H, S, D), dt)
        want = oracle.norms(kn[:, :, ZONE_START:ZONE_START + ZONE_LEN])
        want_bytes = np.ascontiguousarray(want).view(np.uint8).reshape(B * H, ZONE_LEN * esz)
        want_tmax = _tile_maxima(want, dt)
        k, v = to_dev(kn, DEV), to_dev(vn, DEV)
        dense = {}
        for mode in (PT.NORM, PT.SNAPKV):
            ctx = (dt, D, variant, "snapkv" if mode == PT.SNAPKV else "norm", "dense")
            norms, tmax, layout = dense[mode] = _score(dt, D, _spec(mode), k, v, None)
            assert np.array_equal(norms, want_bytes), ctx
            if mode == PT.SNAPKV:
                got = tmax.view(np.uint32).reshape(B * H, -1)[:, :want_tmax.shape[1]]
                assert np.array_equal(got, want_tmax), ctx
        for P in PAGE_SIZES:
            npp = -(-S // P)
            pl = PU.Layer(kn, vn, P, seed + P, table_cols=npp + 3)
            assert npp == 1 or not np.array_equal(np.diff(pl.table_np, axis=1),
                                                   np.ones((B, npp - 1)))  # shuffled
            snap = pl.snapshot()
            for mode in (PT.NORM, PT.SNAPKV):
                ctx = (dt, D, variant, "snapkv" if mode == PT.SNAPKV else "norm", P)
                norms, tmax, layout = _score(dt, D, _spec(mode), None, None, pl)
                assert layout == dense[mode][2], ctx
                assert np.array_equal(norms, dense[mode][0]), ctx + ("paged != dense",)
                assert np.array_equal(norms, want_bytes), ctx + ("paged != oracle",)
                if mode == PT.SNAPKV:
                    assert tmax.size and np.array_equal(tmax, dense[mode][1]), ctx + ("tmax",)
            pl.assert_pools(snap, (dt, D, variant, P))
