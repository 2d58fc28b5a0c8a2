"""Causal attention column sums at their edges (csrc/kvc_colsum.h, colsum_score_impl in
csrc/kvc.hip, kvcompress/methods/colsum.py), every case against test_colsum_gpu.reference: float64
on the CPU from the same rounded 16-bit inputs.

  1. (L, q) pairs at which mb, the split count or a wave-uniform masked / skip test changes value;
  2. sharp and wide-range softmaxes: a running maximum that keeps growing, logits in the tens,
     fp16 sums in the subnormal range, a diagonal that carries most of every row's mass;
  3. more than kColsumLayers = 32 layers in one call, chunks with and without a caller's lse, and
     include/kvc.h's two bit-level promises;
  4. strided Q and the forms of lse the wrapper converts;
  6. capture under torch.cuda.graph, and non-finite inputs.
(5, the direct-ABI tests, is tests/test_colsum_abi_gpu.py.)"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from colsum_util import HKV, params, randn_inputs, scratch_bytes, split, table
from kvcompress import _engine as E
from kvcompress import _native as N
from kvcompress import attention_column_sums
from kvcompress.methods.colsum import column_sums
from test_colsum_args import scratch_formula
from test_colsum_gpu import BF16, BOUND, FP16, case, reference, rel_err

LOG2E = 1.4426950408889634


def checked_reference(k, q, scale=None):
    want, lse = reference(k, q, scale)
    assert want.min() > 1e-30  # normal fp32 numbers: a relative error means something
    return want, lse


# ----------------------------------------------------------------------------------------------
# 1. shape edges.  Maximum relative error over this section, measured on an MI355X: 1.35e-6
# (printed by the tests; the worst case is (2248, 1) at D = 256, five splits merged for one query
# row; the 32-split cap gives 1.10e-6), under test_colsum_gpu's BOUND = 3.1e-6 as it stands.
# ----------------------------------------------------------------------------------------------
# ((L, q), (mb, nsplit)) at B = 1, G = 1, i.e. R = 2 rows; case i has D = DS[i % 4], and its dtype
# alternates with a phase that moves every four cases, so that no D is tied to one dtype
SWEEP = [
    ((1, 1), (1, 1)), ((2, 1), (1, 1)), ((2, 2), (1, 1)),                # smallest shapes
    ((32, 32), (1, 1)), ((33, 33), (2, 1)), ((64, 64), (2, 1)),          # mb 1 -> 2 -> 4 and
    ((65, 65), (4, 1)), ((128, 128), (4, 1)), ((129, 129), (4, 1)),      # tile edges
    ((128, 1), (1, 1)), ((129, 1), (1, 1)), ((2248, 1), (1, 5)),         # mb = 1: one split, five
    ((160, 32), (1, 1)), ((159, 32), (1, 1)), ((161, 32), (1, 1)),       # L - q = 128, 127, 129
    ((96, 64), (2, 1)), ((287, 64), (2, 1)),                             # L - q = 32, = 31 mod 32
    ((256, 128), (4, 1)),                                                # L - q = 128, mb = 4
    ((1100, 48), (2, 3)),                                                # mb = 2, three splits
    ((640, 640), (4, 2)),                                                # 5 tiles, 3 per split
    ((513, 257), (4, 2)),                                                # q = 2 * 128 + 1
    ((16001, 17), (1, 32)),                                              # kColsumMaxSplits
]
DS = (64, 128, 80, 256)


def sweep_case(i):
    return DS[i % 4], (BF16, FP16)[(i + i // 4) % 2]


def test_sweep_covers_what_it_claims():
    """No GPU: the split arithmetic of every sweep case, against test_colsum_args.scratch_formula
    too, and the coverage of D and dtype."""
    for (L, q), (mb, nsplit) in SWEEP:
        got = split(2, q, L)
        assert (got[0], got[4]) == (mb, nsplit), (L, q, got)
        assert scratch_bytes(2, q, L) == scratch_formula(2, q, L)
    assert split(2, 17, 16001) == (1, 1, 126, 4, 32)  # the cap: 32 splits of 4 tiles
    assert split(2, 640, 640)[2:4] == (5, 3)          # tiles is no multiple of tps
    assert split(2, 1, 2248)[2:] == (18, 4, 5)
    combos = [sweep_case(i) for i in range(len(SWEEP))]
    for D in DS:
        assert sum(c[0] == D for c in combos) >= 4 and {c[1] for c in combos if c[0] == D} == \
            {BF16, FP16}
    assert all(sum(c[1] == dt for c in combos) >= 4 for dt in (BF16, FP16))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SWEEP)), ids=["L%d_q%d" % s[0] for s in SWEEP])
def test_shape_edges_against_float64(i):
    (L, ql), (mb, nsplit) = SWEEP[i]
    D, dtype = sweep_case(i)
    got_split = split(2, ql, L)
    assert (got_split[0], got_split[4]) == (mb, nsplit)
    k, q = randn_inputs(100 + i, dtype, 1, 1, L, ql, D)
    want, _ = checked_reference(k, q)
    got = attention_column_sums(k, q)
    assert got.dtype == torch.float32 and got.shape == want.shape
    err = rel_err(got, want)
    print(f"colsum edge (L, q) = ({L}, {ql}), D = {D}, {dtype}: max relative error {err:.3e}")
    assert err < BOUND


# (dtype, B, G, D, L, q, scale)
FURTHER = {
    "g16": (FP16, 1, 16, 64, 200, 40, None),
    "b3_g2": (BF16, 3, 2, 128, 300, 129, None),
    "scale_given": (BF16, 1, 1, 80, 333, 100, 0.11),
    "scale_negative": (FP16, 1, 1, 64, 333, 100, -0.2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FURTHER))
def test_groups_batches_and_scales_against_float64(name):
    dtype, B, G, D, L, ql, scale = FURTHER[name]
    k, q = randn_inputs(150, dtype, B, G, L, ql, D)
    want, _ = checked_reference(k, q, scale)
    err = rel_err(attention_column_sums(k, q, scale=scale), want)
    print(f"colsum {name}: max relative error {err:.3e}")
    assert err < BOUND


@pytest.mark.gpu
def test_callers_lse_with_a_batch_against_float64():
    k, q, want, lse = case("batch2_g3_new_block")  # B = 2, G = 3, (260, 129)
    err = rel_err(attention_column_sums(k, q, lse=lse), want)
    print(f"colsum batch2_g3_new_block lse=True: max relative error {err:.3e}")
    assert err < BOUND


# ----------------------------------------------------------------------------------------------
# 2. sharp and wide-range softmaxes
# ----------------------------------------------------------------------------------------------
# Maximum relative error of the fp32 sums against float64 over SHARP, measured on an MI355X:
# 4.2e-6 over the eight ramps (the worst is ramp_down, bf16, (700, 700)) and 6.5e-7 over the two
# diagonals (printed by the tests).  Each bound is 4x its figure, test_colsum_gpu's margin for
# other seeds and boxes; the two constructions have one each because their logits differ threefold
# in size (|s| log2 e up to ~40 and ~12) and the error grows with it.  BOUND itself cannot hold for
# the ramps: the fp32 roundings of s and lse alone move exp2(s - lse) by 2^-24 |s| ln 2 per term.
# Every test checks that its bound stays under its own a-priori ceiling (sharp()): those came to
# 1.05e-4 ... 2.07e-4 for the ramps and 3.4e-5, 6.6e-5 for the diagonals.
SHARP_BOUND = {"ramp": 1.7e-5, "diagonal": 2.6e-6}
assert max(SHARP_BOUND.values()) < 2.0 ** -12

# (construction, dtype, B, G, D, L, q)
SHARP = {}
for _way in ("ramp_up", "ramp_down"):
    for _dt, _G, _D, _L, _q in ((BF16, 2, 128, 700, 700), (BF16, 2, 128, 700, 200),
                                (FP16, 1, 64, 1100, 1100), (FP16, 1, 64, 1100, 300)):
        SHARP["%s_%s_%d_%d" % (_way, "bf16" if _dt is BF16 else "fp16", _L, _q)] = \
            (_way, _dt, 1, _G, _D, _L, _q)
SHARP["diagonal_bf16_389_389"] = ("diagonal", BF16, 2, 3, 128, 389, 389)
SHARP["diagonal_fp16_389_131"] = ("diagonal", FP16, 1, 1, 64, 389, 131)
RAMP_AMP, DIAGONAL_AMP = 24.0, 8.0


@functools.lru_cache(maxsize=None)
def sharp(name):
    """(k, q, want, float64 lse, ceiling) of a SHARP case.  ceiling = (D + 4) 2^-24 ln 2 A with
    A = scale log2(e) max_ij sum_d |Q_id| |K_jd|: the fp32 accumulation bound of a D-term dot
    product of exactly representable products, plus the roundings of the scale, s, lse and the
    difference, carried through exp2."""
    way, dtype, B, G, D, L, ql = SHARP[name]
    g = torch.Generator().manual_seed(20 + list(SHARP).index(name))
    if way == "diagonal":
        # every query's own key, the last the mask allows, carries most of its mass
        dirs = F.normalize(torch.randn(B, HKV, L, D, generator=g), dim=-1)
        k = D ** 0.5 * dirs
        q = DIAGONAL_AMP * dirs[:, :, L - ql:].repeat_interleave(G, 1) + \
            0.1 * torch.randn(B, HKV * G, ql, D, generator=g)
    else:
        # up: the running maximum grows at nearly every key; down: it is the first key's, and the
        # later keys lie ~70 binades below it
        u = F.normalize(torch.randn(D, generator=g), dim=0)
        t = torch.linspace(-1, 1, L) * (1 if way == "ramp_up" else -1)
        k = t[:, None] * u * D ** 0.5 + 0.25 * torch.randn(B, HKV, L, D, generator=g)
        q = RAMP_AMP * u + 0.25 * torch.randn(B, HKV * G, ql, D, generator=g)
    k, q = k.to(dtype).cuda(), q.to(dtype).cuda()
    want, lse = checked_reference(k, q)
    k64 = k.double().cpu().repeat_interleave(G, 1)
    A = D ** -0.5 * LOG2E * (q.double().cpu().abs() @ k64.abs().transpose(-1, -2)).max().item()
    if way == "diagonal":  # the guard, on the reference alone
        own = (q.double().cpu() * k64[:, :, L - ql:]).sum(-1) * D ** -0.5
        p = (own - lse).exp().mean().item()
        assert 0.5 <= p <= 0.99, p
    return k, q, want, lse, (D + 4) * 2.0 ** -24 * math.log(2) * A


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHARP))
def test_sharp_softmax_against_float64(name):
    k, q, want, _, ceiling = sharp(name)
    err = rel_err(attention_column_sums(k, q), want)
    print(f"colsum {name}: max relative error {err:.3e}, a-priori ceiling {ceiling:.3e}, "
          f"smallest sum {want.min().item():.3e}")
    bound = SHARP_BOUND[SHARP[name][0].split("_")[0]]
    assert bound <= ceiling
    assert err < bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ramp_up_fp16_1100_300", "ramp_down_fp16_1100_300"])
def test_fp16_rows_round_into_subnormals_as_torch_does(name):
    k, q, want, _, _ = sharp(name)
    below = (want < 2.0 ** -14).double().mean().item()  # under the smallest normal fp16
    assert 0.5 <= below <= 0.75, below
    f32, dts = column_sums([k], [q], [None], None, True, True)
    assert dts[0].dtype == FP16 and torch.equal(dts[0], f32[0].to(FP16))
    assert (dts[0] == 0).any() and ((dts[0] > 0) & (dts[0] < 2.0 ** -14)).any()


# ----------------------------------------------------------------------------------------------
# 3. more than 32 layers, mixed lse, and the bit-level promises
# ----------------------------------------------------------------------------------------------
NL = 34  # kColsumLayers + 2: the chunk loop runs twice


@functools.lru_cache(maxsize=None)
def layers34():
    """[(k, q, want, fp32 natural-log lse)] of 34 bf16 layers, B = 1, G = 2, D = 64."""
    out = []
    for i in range(NL):
        L = 40 + 37 * i % 300 + 1
        ql = min((1, 7, 33, 65, L)[i % 5], L)
        k, q = randn_inputs(300 + i, BF16, 1, 2, L, ql, 64)
        want, lse = checked_reference(k, q)
        out.append((k, q, want, lse.float().cuda()))
    return out


@functools.lru_cache(maxsize=None)
def alone(i, with_lse):
    k, q, _, lse = layers34()[i]
    return attention_column_sums(k, q, lse=lse if with_lse else None)


def call34(flags):
    ly = layers34()
    return attention_column_sums([y[0] for y in ly], [y[1] for y in ly],
                                 lse=[y[3] if f else None for y, f in zip(ly, flags)])


def check34(got, flags):
    for i, (_, _, want, _) in enumerate(layers34()):
        assert rel_err(got[i], want) < BOUND, i
        assert torch.equal(got[i], alone(i, flags[i])), f"layer {i}: not its one-layer call's bits"


@pytest.mark.gpu
def test_34_layers_of_mixed_lse_each_as_if_alone_and_twice_the_same():
    flags = [i % 3 == 0 for i in range(NL)]
    got = call34(flags)
    check34(got, flags)
    again = call34(flags)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # layer 33 (with its lse) as layer 0 of a two-layer call beside another shape
    k, q, _, lse = layers34()[33]
    k1, q1 = randn_inputs(399, BF16, 1, 2, 130, 7, 64)
    two = attention_column_sums([k, k1], [q, q1], lse=[lse, None])
    assert torch.equal(two[0], got[33])
    assert rel_err(two[1], reference(k1, q1)[0]) < BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("lse_first", [True, False], ids=["lse_chunk_first", "lse_chunk_last"])
def test_a_chunk_whose_layers_all_bring_lse_skips_the_statistics(lse_first):
    flags = [(i < 32) == lse_first for i in range(NL)]
    ly = layers34()
    outs = [torch.empty_like(y[2], dtype=torch.float32, device="cuda") for y in ly]
    t = table([y[0] for y in ly], [y[1] for y in ly],
              [y[3] if f else None for y, f in zip(ly, flags)], f32=outs)
    R = HKV * 2
    # the scratch of exactly the layers without lse
    assert N.colsum_plan(params(ly[0][0], ly[0][1]), t) == \
        (0, sum(scratch_formula(R, y[1].shape[2], y[0].shape[2])
                for y, f in zip(ly, flags) if not f))
    check34(call34(flags), flags)


# ----------------------------------------------------------------------------------------------
# 4. strided Q and the forms of lse
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype, L, ql", [(BF16, 300, 129), (FP16, 200, 32)])
@pytest.mark.parametrize("kind", ["tail_view", "fused_third", "last_dim_strided"])
def test_strided_queries_against_float64(kind, dtype, L, ql):
    B, G, D = 2, 2, 128
    g = torch.Generator().manual_seed(40)
    k = torch.randn(B, HKV, L, D, generator=g).to(dtype).cuda()
    if kind == "tail_view":  # the last q rows of a full-length projection
        q = torch.randn(B, HKV * G, L, D, generator=g).to(dtype).cuda()[:, :, L - ql:L]
    elif kind == "fused_third":  # the first third of a [B, q, 3, Hq, D] projection output
        q = torch.randn(B, ql, 3, HKV * G, D, generator=g).to(dtype).cuda()[:, :, 0]
        q = q.permute(0, 2, 1, 3)
    else:
        q = torch.randn(B, HKV * G, ql, 2 * D, generator=g).to(dtype).cuda()[..., ::2]
    assert not q.is_contiguous()
    # the kernels read the first two as they lie; the third goes through the wrapper's copy
    assert E._takes_as_is(q) == (kind != "last_dim_strided")
    want, _ = checked_reference(k, q)
    err = rel_err(attention_column_sums(k, q), want)
    print(f"colsum q {kind} ({L}, {ql}) {dtype}: max relative error {err:.3e}")
    assert err < BOUND


@pytest.mark.gpu
def test_lse_of_any_floating_form_is_its_float32_values():
    k, q, _, lse = case("batch2_g3_new_block")
    base = attention_column_sums(k, q, lse=lse)
    lse64 = reference(k, q)[1].cuda()
    assert lse64.dtype == torch.float64 and torch.equal(lse64.float(), lse)
    assert torch.equal(attention_column_sums(k, q, lse=lse64), base)
    wide = torch.zeros(*lse.shape, 2, device="cuda")
    wide[..., 0] = lse
    assert not wide[..., 0].is_contiguous()
    assert torch.equal(attention_column_sums(k, q, lse=wide[..., 0]), base)
    rounded = lse.to(BF16)
    assert not torch.equal(rounded.float(), lse)
    assert torch.equal(attention_column_sums(k, q, lse=rounded),
                       attention_column_sums(k, q, lse=rounded.float()))


# ----------------------------------------------------------------------------------------------
# 6. graph capture and non-finite inputs
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capture_and_replay_match_eager_bit_for_bit():
    """One stream, no branches: a layer with lse and one without, captured once and replayed over
    refilled K, Q and lse (the warm-up and refill protocol of tests/test_graph_capture.py)."""
    shapes = ((300, 129), (130, 7))

    def fill(n):
        kq = [randn_inputs(600 + 10 * n + li, BF16, 2, 2, L, ql, 128)
              for li, (L, ql) in enumerate(shapes)]
        return kq, reference(*kq[0])[1].float().cuda()

    (kq, lse) = fill(0)
    ks, qs = [k.clone() for k, _ in kq], [q.clone() for _, q in kq]
    lse = lse.clone()
    run = lambda: attention_column_sums(ks, qs, lse=[lse, None])  # noqa: E731
    run()  # the warm-up: an eager call loads the kernels
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    seen = []
    for n in (1, 2):
        kq, new_lse = fill(n)
        for dst, src in zip(ks + qs + [lse], [k for k, _ in kq] + [q for _, q in kq] + [new_lse]):
            dst.copy_(src)
        for o in out:
            o.fill_(-1.0)
        g.replay()
        got = [o.clone() for o in out]
        eager = run()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, eager)), f"fill {n}"
        assert rel_err(got[1], reference(*kq[1])[0]) < BOUND
        seen.append(got)
    assert not torch.equal(seen[0][0], seen[1][0])  # the fills cannot be mistaken for one another


@pytest.mark.gpu
def test_non_finite_inputs_spoil_their_own_heads_only():
    G = 2
    k, q = randn_inputs(70, BF16, 2, G, 300, 129, 128)
    clean = attention_column_sums(k, q)
    kp, qp = k.clone(), q.clone()
    kp[0, 0, 5, 3], kp[0, 0, 150, 0], kp[0, 0, 299, 7] = float("nan"), float("inf"), float("-inf")
    qp[0, 1, 64, 2] = float("nan")  # query head 1 of G = 2: KV head 0's group
    got = attention_column_sums(kp, qp)
    torch.cuda.synchronize()  # the call returned; no kernel faulted
    assert torch.equal(got[:, G:], clean[:, G:])  # every query head of KV head 1
    assert torch.equal(got[1], clean[1])          # and the batch beside the poisoned one
    # (nothing is asserted about batch 0's heads 0 and 1: their sums are unspecified)
