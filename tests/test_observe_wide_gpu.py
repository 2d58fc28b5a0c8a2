"""Observation-window scores of wide query groups (csrc/kvc_observe_wide.h: any G <= 16 with
M = G * W <= 256, MB = ceil(M / 32) query blocks): against the float64 reference, bit for bit
across key sources, and snapkv_compress / snapkv_compress_paged end to end on planted keys."""
import pytest
import torch

import fp8_gpu as F8
import paged_util as PU
from gpu_util import to_np
from kvcompress import observation_scores, snapkv_compress, snapkv_compress_paged
from test_observe_gpu import BF16, BOUND, FP16, inputs, planted, reference, rel_err

pytestmark = pytest.mark.gpu
# Maximum relative error of the fp32 scores against float64 over CASES, measured on an MI355X:
# 3.7e-7 (printed by the test; the worst case is MB = 6 with the mask across a chunk edge).  That is
# below a quarter of the project's BOUND = 1.9e-6 (4x the 4.8e-7 measured for M <= 128): kept.
assert BOUND < 2.0 ** -12

# (dtype, B, G, W, D, S, zone, P, mode, scale); H = 2.  Chunks are 1 024 keys, tiles 128.
CASES = {
    "g3_half_block_ragged_tile": (FP16, 1, 3, 16, 64, 333, (0, None), 5, "avg", None),
    "mb3_first_odd": (BF16, 1, 3, 32, 128, 200, (3, None), 3, "avg", None),
    "mb3_half_block": (FP16, 1, 5, 16, 64, 333, (0, None), 5, "avg", None),
    "mb5_one_wave_owns_two": (BF16, 1, 5, 32, 128, 129, (0, None), 1, "max", None),
    "mb6_mask_across_a_chunk_edge": (BF16, 1, 6, 32, 64, 1100, (0, None), 1, "max", None),
    "mb7_batch2_zone_start": (BF16, 2, 7, 32, 128, 700, (37, 500), 5, "max", None),
    "mb8_two_chunks_and_a_third": (BF16, 1, 8, 32, 128, 2248, (0, None), 7, "max", None),
    "g16_d256_zone_shorter_than_pool": (FP16, 1, 16, 16, 256, 150, (10, 14), 7, "avg", None),
    "w64_full_width_scale_given": (FP16, 1, 4, 64, 128, 129, (0, None), 7, "avg", 0.11),
}


@pytest.mark.parametrize("name", list(CASES))
def test_scores_against_float64(name):
    dtype, B, G, W, D, S, zone, P, mode, scale = CASES[name]
    k, q = inputs(1, dtype, B, 2, G, S, W, D)
    got = observation_scores(k, q, zone=zone, pooling_kernel=P, pooling=mode, scale=scale)
    want = reference(k, q, zone, P, mode, scale)
    assert got.dtype == torch.float32 and got.shape == want.shape
    err = rel_err(got, want)
    print(f"observe wide {name}: max relative error {err:.3e}")
    assert err < BOUND


@pytest.mark.parametrize("G, W, D", [(7, 32, 128), (8, 32, 64)])
def test_sources_bit_for_bit(G, W, D):
    """Paged keys give the dense call's bits; fp8 keys those of the bf16 call on the upcast."""
    k, q = inputs(5, BF16, 1, 2, G, 1100, W, D)
    dense = observation_scores(k, q, pooling_kernel=5)
    for P in (16, 256):
        pl = PU.Layer(to_np(k), to_np(k), P, 11 + P)
        assert torch.equal(observation_scores(pl.paged, q, pooling_kernel=5), dense)
    for fmt, f8 in (("e4m3", torch.float8_e4m3fn), ("e5m2", torch.float8_e5m2)):
        k8 = k.to(f8)
        up = observation_scores(k8.to(BF16), q, pooling_kernel=5)
        pool = F8.Pool((F8.as_u8(k8).cpu().numpy(),) * 2, fmt, 16, 13)
        assert torch.equal(observation_scores(k8, q, pooling_kernel=5), up)
        assert torch.equal(observation_scores(pool.paged(), q, pooling_kernel=5), up)


@pytest.mark.parametrize("dtype, D, S, W, G, P, n, sink, paged", [
    (BF16, 128, 400, 32, 8, 5, 9, 4, True), (FP16, 64, 333, 16, 5, 5, 8, 0, False),
    (BF16, 128, 1100, 32, 7, 7, 10, 0, True), (BF16, 256, 200, 16, 16, 1, 6, 0, False),
    (BF16, 128, 300, 32, 3, 3, 8, 0, False), (BF16, 64, 1300, 64, 4, 5, 10, 2, False)])
def test_planted_keys_end_to_end(dtype, D, S, W, G, P, n, sink, paged):
    B, H, keep = 2, 2, n * P
    k, v, q, pos = planted(3, dtype, B, H, G, S, W, D, P, n, sink)
    # the guard, on the float64 reference alone: the keep-th score is >= 8x the next one, so the
    # kept set depends neither on rounding nor on tie order
    ref = reference(k, q, (sink, None), P, "avg").sort(-1, descending=True).values
    assert (ref[..., keep - 1] / ref[..., keep]).min() >= 8
    idx = (pos[..., None] + torch.arange(-(P // 2), P // 2 + 1)).flatten(2)
    idx = torch.cat([torch.arange(sink).expand(B, H, sink), idx], 2).cuda()
    want = [torch.cat([x.gather(2, idx[..., None].expand(-1, -1, -1, D)), x[:, :, -W:]], 2)
            for x in (k, v)]
    kw = dict(observation_window=W, keep_size=sink + keep + W, pooling_kernel=P, sink_size=sink)
    out = snapkv_compress([(k, v)], [q], **kw)
    for got, w in zip(out[0], want):
        assert got.shape == w.shape and torch.equal(got.view(torch.int16), w.view(torch.int16))
    if paged:  # in place behind a shuffled table: the pools whole, dense result scattered
        pl = PU.Layer(to_np(k), to_np(v), 16, 21)
        snap = pl.snapshot()
        assert snapkv_compress_paged([pl.paged], [q], **kw) == [sink + keep + W]
        pl.expect(snap, *(to_np(w) for w in want))
        pl.assert_pools(snap, (str(dtype), 16))
