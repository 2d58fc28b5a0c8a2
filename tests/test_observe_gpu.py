"""Observation-window (SnapKV) scores on the GPU: the MFMA kernel set of csrc/kvc_observe.h
against include/kvc.h's formulas in torch float64 on the CPU, on the same bf16 / fp16 inputs;
snapkv_compress end to end on planted keys; its early returns against snapkv_lite_compress."""
import pytest
import torch
import torch.nn.functional as F

from kvcompress import observation_scores, snapkv_compress
from kvcompress.methods import snapkv_lite_compress

BF16, FP16 = torch.bfloat16, torch.float16
# Maximum relative error of the fp32 scores against float64 over the cases below, measured on an
# MI355X: 4.8e-7 (printed by the test; the worst case is the three-chunk one).  The bound is 4x
# that -- the margin for other seeds and boxes -- and far below the 2^-12 (2.4e-4) that would let a
# stored bf16 / fp16 score leave its ulp.
BOUND = 1.9e-6
assert BOUND < 2.0 ** -12


def reference(k, q, zone, P, mode, scale=None):
    """float64 [B, Hkv, zone_len]: the contract of include/kvc.h, "Observation-window scores"."""
    (B, H, S, D), (Hq, W) = k.shape, q.shape[1:3]
    k64, q64 = k.double().cpu(), q.double().cpu().view(B, H, Hq // H, W, D)
    s = torch.einsum("bhgid,bhjd->bhgij", q64, k64) * (scale or D ** -0.5)
    allowed = torch.arange(S)[None, :] <= (S - W + torch.arange(W))[:, None]
    p = torch.softmax(s.masked_fill(~allowed, float("-inf")), -1)
    imp = p.sum((2, 3))[:, :, range(S - W)[zone[0]:zone[1]]]
    pool = F.avg_pool1d if mode == "avg" else F.max_pool1d
    return pool(imp, P, 1, P // 2)


def inputs(seed, dtype, B, H, G, S, W, D, fused=False):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, G * H, W, D, generator=g).to(dtype).cuda()
    if fused:  # K as the strided middle third of a [B, S, 3, H, D] projection output
        k = torch.randn(B, S, 3, H, D, generator=g).to(dtype).cuda()[:, :, 1].permute(0, 2, 1, 3)
        assert not k.is_contiguous()
        return k, q
    return torch.randn(B, H, S, D, generator=g).to(dtype).cuda(), q


# (dtype, B, G, S, W, D, zone, P, mode, fused); H = 2.  Chunks are 1 024 keys, tiles 128.
CASES = {
    "zone_len_1": (BF16, 1, 1, 33, 32, 128, (0, None), 1, "avg", False),
    "ragged_tile_m16_fp16": (FP16, 1, 1, 333, 16, 64, (0, None), 5, "avg", False),
    "two_chunks_and_a_third": (BF16, 1, 2, 2248, 32, 128, (0, None), 7, "max", False),
    "m128_zone_start_batch2": (BF16, 2, 2, 700, 64, 128, (37, 500), 5, "max", False),
    "d256_m128_zone_shorter_than_pool": (FP16, 1, 8, 150, 16, 256, (10, 14), 7, "avg", False),
    "mask_across_a_chunk_edge": (BF16, 1, 4, 1100, 32, 64, (0, None), 1, "max", False),
    "fused_qkv_third": (BF16, 2, 1, 200, 32, 128, (3, None), 3, "avg", True),
    "scale_given": (FP16, 1, 2, 129, 64, 128, (0, None), 7, "avg", False),
}


def rel_err(got, want):
    return ((got.double().cpu() - want).abs() / want).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_scores_against_float64(name):
    dtype, B, G, S, W, D, zone, P, mode, fused = CASES[name]
    k, q = inputs(1, dtype, B, 2, G, S, W, D, fused)
    scale = 0.11 if name == "scale_given" else None
    got = observation_scores(k, q, zone=zone, pooling_kernel=P, pooling=mode, scale=scale)
    want = reference(k, q, zone, P, mode, scale)
    assert got.dtype == torch.float32 and got.shape == want.shape
    err = rel_err(got, want)
    print(f"observe {name}: max relative error {err:.3e}")
    assert err < BOUND


@pytest.mark.gpu
def test_two_layers_of_different_length_in_one_call():
    ks, qs = zip(*(inputs(2 + i, BF16, 1, 2, 2, S, 32, 128) for i, S in enumerate((130, 1300))))
    got = observation_scores(ks, qs, pooling_kernel=5)
    for i, (k, q) in enumerate(zip(ks, qs)):
        err = rel_err(got[i], reference(k, q, (0, None), 5, "avg"))
        print(f"observe two layers, layer {i}: max relative error {err:.3e}")
        assert err < BOUND


def planted(seed, dtype, B, H, G, S, W, D, P, n, sink=0):
    """K, V, Q and the planted prefix positions [B, H, n] (the recipe of the planted-key test)."""
    g = torch.Generator().manual_seed(seed)
    u = F.normalize(torch.randn(B, H, 1, D, generator=g), dim=-1)
    q = 6 * u.repeat_interleave(G, 1) + 0.5 * torch.randn(B, G * H, W, D, generator=g)
    k, v = torch.randn(B, H, S, D, generator=g), torch.randn(B, H, S, D, generator=g)
    spacing = (S - W - sink - P) // n
    assert spacing >= 2 * P + 1
    off = torch.randint(0, spacing - 2 * P, (B, H, 1), generator=g)
    pos = sink + P // 2 + off + spacing * torch.arange(n)
    k.scatter_add_(2, pos[..., None].expand(B, H, n, D), (8 * D ** 0.5 / 6) * u.expand(B, H, n, D))
    return k.to(dtype).cuda(), v.to(dtype).cuda(), q.to(dtype).cuda(), pos


@pytest.mark.gpu
@pytest.mark.parametrize("dtype, D, S, W, G, P, n, sink", [
    (BF16, 128, 200, 32, 1, 1, 12, 0), (FP16, 64, 333, 16, 4, 5, 8, 0),
    (BF16, 128, 1100, 64, 2, 7, 10, 0), (BF16, 256, 129, 32, 1, 5, 4, 0),
    (BF16, 128, 400, 32, 2, 5, 9, 4)])
def test_planted_keys_end_to_end(dtype, D, S, W, G, P, n, sink):
    B, H, keep = 2, 2, n * P
    k, v, q, pos = planted(3, dtype, B, H, G, S, W, D, P, n, sink)
    # the guard, on the float64 reference alone: the keep-th score is >= 8x the next one, so the
    # kept set depends neither on rounding nor on tie order
    ref = reference(k, q, (sink, None), P, "avg").sort(-1, descending=True).values
    assert (ref[..., keep - 1] / ref[..., keep]).min() >= 8
    idx = (pos[..., None] + torch.arange(-(P // 2), P // 2 + 1)).flatten(2)
    idx = torch.cat([torch.arange(sink).expand(B, H, sink), idx], 2).cuda()
    other = tuple(t.clone() for t in (k, v))  # a skipped layer beside the compressed one
    out = snapkv_compress([(k, v), other], [q, q], observation_window=W,
                          keep_size=sink + keep + W, pooling_kernel=P, sink_size=sink,
                          skip_layers=[1])
    assert out[1] is other
    for x, got in zip((k, v), out[0]):
        want = torch.cat([x.gather(2, idx[..., None].expand(-1, -1, -1, D)), x[:, :, -W:]], 2)
        assert got.shape == want.shape and torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("S, keep, W", [(40, 64, 16), (64, 64, 16), (20, 10, 32), (100, 32, 32),
                                        (100, 20, 32)])
def test_early_returns_match_snapkv_lite(S, keep, W):
    """seq_len <= keep_size, a non-positive prefix and keep_size <= window: the same objects /
    views as snapkv_lite_compress (no engine call: CPU tensors do)."""
    kv = [(torch.zeros(1, 2, S, 64, dtype=BF16), torch.ones(1, 2, S, 64, dtype=BF16))]
    q = [torch.zeros(1, 2, W, 64, dtype=BF16)]
    got = snapkv_compress(list(kv), q, observation_window=W, keep_size=keep)
    want = snapkv_lite_compress(list(kv), observation_window=W, keep_size=keep)
    for (a, b), (c, d), (k, v) in zip(got, want, kv):
        assert (a is k and b is v) == (c is k and d is v)
        for x, y in ((a, c), (b, d)):
            assert (x.data_ptr(), x.shape, x.stride()) == (y.data_ptr(), y.shape, y.stride())
