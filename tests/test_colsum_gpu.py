"""Causal attention column sums on the GPU: the MFMA kernel set of csrc/kvc_colsum.h against
include/kvc.h's formulas in torch float64 on the CPU, on the same bf16 / fp16 inputs; then
H2OAttentionManager.update_from_queries + h2o_attention_compress end to end on planted heavy
hitters, and its composition with update_attention_scores."""
import functools

import pytest
import torch
import torch.nn.functional as F

from kvcompress import attention_column_sums
from kvcompress.methods.colsum import column_sums
from kvcompress.methods.h2o_attention import H2OAttentionManager, h2o_attention_compress

BF16, FP16 = torch.bfloat16, torch.float16
# Maximum relative error of the fp32 sums against float64 over the cases below, measured on an
# MI355X: 7.8e-7 (printed by the tests; the worst case is the B = 2, G = 3 one).  The bound is 4x
# that -- the margin for other seeds and boxes -- and far below the 2^-12 (2.4e-4) that would let a
# stored bf16 / fp16 sum leave its ulp.
BOUND = 3.1e-6
assert BOUND < 2.0 ** -12

# (dtype, B, G, L, q, D, fused); Hkv = 2.  Key chunks and query tiles are 128 rows, blocks 32.
CASES = {
    "decode_row": (BF16, 1, 1, 33, 1, 128, False),
    "full_prefill_fp16": (FP16, 1, 1, 333, 333, 64, False),
    "mask_mid_tile": (BF16, 1, 2, 1100, 300, 128, False),
    "chunks_blocks_splits": (BF16, 1, 1, 2248, 2248, 128, False),
    "d256_group": (FP16, 1, 4, 150, 40, 256, False),
    "d80": (BF16, 1, 1, 200, 200, 80, False),
    "batch2_g3_new_block": (BF16, 2, 3, 260, 129, 128, False),
    "fused_qkv_third": (BF16, 2, 1, 200, 32, 128, True),
}


def reference(k, q, scale=None):
    """float64 (imp [B, Hq, L], lse [B, Hq, q]): the contract of include/kvc.h."""
    (B, H, L, D), (Hq, ql) = k.shape, q.shape[1:3]
    k64 = k.double().cpu().repeat_interleave(Hq // H, 1)
    s = q.double().cpu() @ k64.transpose(-1, -2) * (scale or D ** -0.5)
    allowed = torch.arange(L)[None, :] <= (L - ql + torch.arange(ql))[:, None]
    s = s.masked_fill(~allowed, float("-inf"))
    return torch.softmax(s, -1).sum(2), torch.logsumexp(s, -1)


@functools.lru_cache(maxsize=None)
def case(name, seed=1):
    dtype, B, G, L, ql, D, fused = CASES[name]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, 2 * G, ql, D, generator=g).to(dtype).cuda()
    if fused:  # K as the strided middle third of a [B, L, 3, H, D] projection output
        k = torch.randn(B, L, 3, 2, D, generator=g).to(dtype).cuda()[:, :, 1].permute(0, 2, 1, 3)
        assert not k.is_contiguous()
    else:
        k = torch.randn(B, 2, L, D, generator=g).to(dtype).cuda()
    want, lse = reference(k, q)
    assert want.min() > 1e-30  # normal fp32 numbers: a relative error means something
    return k, q, want, lse.float().cuda()


def rel_err(got, want):
    return ((got.double().cpu() - want).abs() / want).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("name, with_lse", [(n, False) for n in CASES] +
                         [("mask_mid_tile", True), ("full_prefill_fp16", True)])
def test_sums_against_float64(name, with_lse):
    k, q, want, lse = case(name)
    got = attention_column_sums(k, q, lse=lse if with_lse else None)
    assert got.dtype == torch.float32 and got.shape == want.shape
    err = rel_err(got, want)
    print(f"colsum {name} lse={with_lse}: max relative error {err:.3e}")
    assert err < BOUND


@pytest.mark.gpu
def test_two_layers_of_different_shape_in_one_call():
    k0, q0, want0, _ = case("mask_mid_tile")  # (L, q) = (1100, 300), beside (130, 7)
    g = torch.Generator().manual_seed(2)
    k1 = torch.randn(1, 2, 130, 128, generator=g).to(BF16).cuda()
    q1 = torch.randn(1, 4, 7, 128, generator=g).to(BF16).cuda()
    got = attention_column_sums([k0, k1], [q0, q1])
    for i, want in enumerate((want0, reference(k1, q1)[0])):
        err = rel_err(got[i], want)
        print(f"colsum two layers, layer {i}: max relative error {err:.3e}")
        assert err < BOUND


@pytest.mark.gpu
def test_dtype_rows_are_the_fp32_rows_rounded():
    k, q, _, _ = case("batch2_g3_new_block")
    f32, dts = column_sums([k], [q], [None], None, True, True)
    assert dts[0].dtype == BF16 and torch.equal(dts[0], f32[0].to(BF16))


# (B, Hkv, G, L, q, D, n, start, recent)
PLANTED = [(1, 2, 1, 700, 700, 64, 8, 4, 64), (1, 2, 2, 1100, 300, 128, 6, 4, 100),
           (1, 2, 4, 333, 333, 64, 5, 2, 40), (1, 2, 1, 2248, 1, 128, 8, 4, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PLANTED)
def test_planted_heavy_hitters_end_to_end(shape):
    B, H, G, L, ql, D, n, start, recent = shape
    g = torch.Generator().manual_seed(3)
    u = F.normalize(torch.randn(B, H, 1, D, generator=g), dim=-1)
    q = 6 * u.repeat_interleave(G, 1) + 0.5 * torch.randn(B, G * H, ql, D, generator=g)
    k, v = torch.randn(B, H, L, D, generator=g), torch.randn(B, H, L, D, generator=g)
    mid = L - recent - start
    pos = start + (torch.arange(n) * mid + mid // 2) // n  # evenly spaced, shared by the heads
    k[:, :, pos] += 8 * D ** 0.5 / 6 * u
    k, v, q = k.to(BF16).cuda(), v.to(BF16).cuda(), q.to(BF16).cuda()
    # guard, on the float64 reference alone: the planted scores stand clear of the rest
    score = reference(k, q)[0].to(BF16).double().sum(1)[0, start:L - recent]
    top = score.sort(descending=True)
    assert top.values[n - 1] >= 2 * top.values[n] and set(top.indices[:n].tolist()) == \
        set((pos - start).tolist())
    mgr = H2OAttentionManager(start_size=start, heavy_hitter_size=n, recent_size=recent,
                              num_heads=G * H)
    mgr.update_from_queries([q], [(k, v)])
    (ko, vo), = h2o_attention_compress([(k, v)], None, mgr, start_size=start,
                                       heavy_hitter_size=n, recent_size=recent)
    keep = torch.cat([torch.arange(start), pos, torch.arange(L - recent, L)]).cuda()
    assert torch.equal(ko, k[:, :, keep]) and torch.equal(vo, v[:, :, keep])


@pytest.mark.gpu
def test_prefill_then_decode_composes_with_update_attention_scores():
    g = torch.Generator().manual_seed(4)
    k = [torch.randn(1, 2, 301, 64, generator=g).to(FP16).cuda() for _ in range(2)]
    q = [torch.randn(1, 4, 301, 64, generator=g).to(FP16).cuda() for _ in range(2)]
    a, b = H2OAttentionManager(num_heads=4), H2OAttentionManager(num_heads=4)
    for L, ql in ((300, 300), (301, 1)):  # a prefill, then one decode step
        ks, qs = [x[:, :, :L] for x in k], [x[:, :, L - ql:L] for x in q]
        a.update_from_queries(qs, [(x, x) for x in ks])
        b.update_attention_scores([s.to(FP16)[:, :, None] for s in attention_column_sums(ks, qs)])
        assert a.current_seq_len == b.current_seq_len == L
        for i in range(2):
            assert a.accumulated_attention[i].dtype == FP16
            assert torch.equal(a.accumulated_attention[i], b.accumulated_attention[i])
