"""Observation-window scores of paged and fp8 caches (kvc_observe_score_paged): bit for bit the
dense bf16 / fp16 call's, no table read past the sequence, a bad page id reported and contained,
and snapkv_compress_paged end to end on planted keys, pools compared whole."""
import numpy as np
import pytest
import torch

import fp8_gpu as F8
import paged_util as PU
from gpu_util import to_np
from kvcompress import PagedKV, _native as N, observation_scores, snapkv_compress, \
    snapkv_compress_paged
from kvcompress.methods.snapkv import _paged_table
from test_observe_gpu import BF16, BOUND, FP16, inputs, planted, reference, rel_err

pytestmark = pytest.mark.gpu
FP8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
NHPD, NPHD = "nhpd", "nphd"


def layer(k, P, seed, **kw):
    return PU.Layer(to_np(k), to_np(k), P, seed, **kw)


# (P, S, dtype, D, W, G, B, zone, K storage, surplus table columns); H = 2, chunks 1 024, tiles 128
@pytest.mark.parametrize("P, S, dtype, D, W, G, B, zone, storage, surplus", [
    (1, 333, FP16, 64, 16, 1, 1, (0, None), NHPD, 0),        # M = 16; 333 staged entries
    (16, 1100, BF16, 64, 32, 4, 1, (0, None), NPHD, 3),      # mask across a chunk edge; 5 of 64
    (256, 2248, BF16, 128, 32, 2, 1, (0, None), NPHD, 0),    # page spans tiles, chunk spans pages
    (2048, 1300, BF16, 128, 32, 1, 1, (0, None), NHPD, 0),   # a page spans chunks
    (16, 700, BF16, 128, 64, 2, 2, (37, 500), NHPD, 0),      # two table rows, zone starts mid-page
    (128, 300, FP16, 256, 16, 8, 1, (0, None), NPHD, 0),     # a tile is a page; D = 256
    (16, 300, FP16, 256, 16, 2, 2, (0, None), NHPD, 1)])
def test_paged_scores_are_the_dense_scores(P, S, dtype, D, W, G, B, zone, storage, surplus):
    """... and entries past ceil(S / P) (out-of-range ids) are not read: the scores do not move
    and the status word stays clear (the suite's per-test check)."""
    k, q = inputs(5, dtype, B, 2, G, S, W, D)
    pl = layer(k, P, 11, k_storage=storage, table_cols=-(-S // P) + surplus)
    kw = dict(zone=zone, pooling_kernel=5)
    dense, paged = observation_scores(k, q, **kw), observation_scores(pl.paged, q, **kw)
    assert paged.dtype == torch.float32 and torch.equal(paged, dense)
    err = rel_err(paged, reference(k, q, zone, 5, "avg"))
    print(f"observe paged P={P} S={S}: max relative error {err:.3e}")
    assert err < BOUND


def test_a_bad_page_id_is_clamped_and_reported():
    """Through the C entry with a status word of the test's own: KVC_DEV_INDEX_RANGE, the run
    completes, and the rows of the batch row whose pages are good keep their bits."""
    B, H, S, W, D = 2, 2, 300, 32, 128
    k, q = inputs(6, BF16, B, H, 1, S, W, D)
    pl = layer(k, 16, 12)
    table, tables = _paged_table([pl.paged], [(0, S - W, 0, 0, 0, 0)])
    status = torch.zeros(1, dtype=torch.int32, device=PU.DEV)
    p = N.Params(dtype=N.KVC_BF16, batch=B, heads=H, head_dim=D, order=N.KVC_DESC,
                 algo=N.KVC_ALGO_TOPK, phases=N.PHASE_ALL, device_status=status.data_ptr())
    rc, info = N.plan_paged(p, table, tables.pages)
    assert rc == 0
    ot = np.zeros(1, dtype=N.OBSERVE_LAYER_DTYPE)
    ot[0] = (q.data_ptr(), q.stride()[:3], 0)
    op = N.ObserveParams(q_heads=H, window=W, pool_kernel=1, scores_row_stride=320)
    rc, sbytes = N.observe_plan_paged(p, op, table, ot, tables.pages)
    assert rc == 0
    ws, scratch = (torch.empty(int(n) + 256, dtype=torch.uint8, device=PU.DEV)
                   for n in (info.workspace_bytes, sbytes))
    got = []
    for bad in (False, True):
        if bad:
            pl.table[0, 5] = pl.k.size(0)  # one past the pool, inside sequence 0
        f32 = torch.zeros(B * H, 320, device=PU.DEV)
        assert N.observe_score_paged(p, op, table, ot, tables.pages, ws.data_ptr(),
                                     int(info.workspace_bytes), scratch.data_ptr(), sbytes,
                                     f32.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        got.append((f32, int(status.item())))
    assert got[0][1] == 0 and got[1][1] == N.DEV_INDEX_RANGE
    assert torch.equal(got[0][0][:, :S - W], observation_scores(k, q).flatten(0, 1))
    assert torch.equal(got[1][0][H:], got[0][0][H:])


@pytest.mark.parametrize("P", [None, 16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("fmt", list(FP8))
def test_fp8_scores_are_the_bf16_scores_of_the_upcast(fmt, D, P):
    k, q = inputs(7, BF16, 1, 2, 2, 1200, 32, D)
    k8 = k.to(FP8[fmt])  # values the format represents; no NaN
    keys = k8 if P is None else F8.Pool((F8.as_u8(k8).cpu().numpy(),) * 2, fmt, P, 13).paged()
    assert torch.equal(observation_scores(keys, q, pooling_kernel=3),
                       observation_scores(k8.to(BF16), q, pooling_kernel=3))


@pytest.mark.parametrize("dtype, P, D, S, W, G, n, sink", [
    (BF16, 16, 128, 400, 32, 2, 9, 4), (FP16, 1, 64, 333, 16, 4, 8, 0),
    ("e4m3", 128, 128, 400, 32, 1, 9, 4), ("e5m2", None, 64, 333, 16, 2, 8, 0)])
def test_planted_keys_end_to_end(dtype, P, D, S, W, G, n, sink):
    B, H, pk, keep = 2, 2, 5, n * 5
    f8 = FP8.get(dtype)
    k, v, q, pos = planted(3, BF16 if f8 else dtype, B, H, G, S, W, D, pk, n, sink)
    if f8:
        k, v = k.to(f8), v.to(f8)
    ref = reference(k, q, (sink, None), pk, "avg").sort(-1, descending=True).values
    assert (ref[..., keep - 1] / ref[..., keep]).min() >= 8  # the kept set is rounding-proof
    idx = (pos[..., None] + torch.arange(-(pk // 2), pk // 2 + 1)).flatten(2)
    idx = torch.cat([torch.arange(sink).expand(B, H, sink), idx], 2).cuda()
    u8 = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731
    want = [torch.cat([x.gather(2, idx[..., None].expand(-1, -1, -1, D)), x[:, :, -W:]], 2)
            for x in (k, v)]
    kw = dict(observation_window=W, keep_size=sink + keep + W, pooling_kernel=pk, sink_size=sink,
              skip_layers=[1])
    if P is None:  # dense fp8 through snapkv_compress: the fp8 dtype and bytes are kept
        out = snapkv_compress([(k, v), (k, v)], [q, q], **kw)
        assert out[1][0] is k and all(g.dtype == f8 and torch.equal(u8(g), u8(w))
                                      for g, w in zip(out[0], want))
        return
    rows = [u8(t).cpu().numpy() if f8 else to_np(t) for t in (k, v)]
    pls = [F8.Pool(tuple(rows), dtype, P, s) if f8 else PU.Layer(*rows, P, s) for s in (21, 22)]
    pks = [pl.paged() if f8 else pl.paged for pl in pls]
    snaps = [pl.snapshot() for pl in pls]
    assert snapkv_compress_paged(pks, [q, q], **kw) == [sink + keep + W, S]
    for got, w in zip(pks[0].to_dense(sink + keep + W), want):
        assert torch.equal(u8(got), u8(w))
    wk, wv = (u8(w).cpu().numpy() if f8 else to_np(w) for w in want)
    for b in range(B if f8 else 1):  # (a Pool takes its expected rows per sequence)
        pls[0].expect(snaps[0], *((b, wk[b:b + 1], wv[b:b + 1]) if f8 else (wk, wv)))
    for pl, snap in zip(pls, snaps):
        pl.assert_pools(snap, (str(dtype), P))


@pytest.mark.parametrize("what, error", [("ragged", TypeError), ("scaled", TypeError),
                                         ("fp8_fp16_queries", TypeError),
                                         ("out", NotImplementedError)])
def test_refused_before_any_launch(what, error):
    f8 = what in ("scaled", "fp8_fp16_queries")
    pool = torch.zeros(8, 2, 16, 64, device=PU.DEV).to(FP8["e4m3"] if f8 else BF16)
    table = torch.arange(8, dtype=torch.int32, device=PU.DEV).view(2, 4)
    scale = torch.ones(8, 2, 16, device=PU.DEV) if what == "scaled" else None
    pk = PagedKV(pool, pool.clone(), table, [60, 50] if what == "ragged" else 60, k_scale=scale)
    q = torch.zeros(2, 2, 16, 64, dtype=FP16 if what == "fp8_fp16_queries" else BF16,
                    device=PU.DEV)
    kw = dict(out=[None]) if what == "out" else {}
    with pytest.raises(error):
        snapkv_compress_paged([pk], [q], observation_window=16, keep_size=32, **kw)
    if what != "out":
        with pytest.raises(error):
            observation_scores(pk, q)
    assert not pool.view(torch.uint8).any()
