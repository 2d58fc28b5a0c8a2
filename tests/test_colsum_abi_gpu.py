"""kvc_colsum_plan / kvc_colsum_score called directly with a numpy layer table (the fields that
kvcompress/methods/colsum.py never sets): padded output rows with both outputs, stray writes into
the gaps, the tail and around an exact-size scratch, and the refusals of colsum_score_impl
(csrc/kvc.hip), which come before anything is enqueued."""
import pytest
import torch

from colsum_util import HKV, params, randn_inputs, scratch_bytes, table
from kvcompress import _native as N
from kvcompress import attention_column_sums
from test_colsum_gpu import BF16, BOUND, reference, rel_err

pytestmark = pytest.mark.gpu

E_ALIGN, E_WORKSPACE = -4, -6  # enum kvc_status, include/kvc.h
SENT32, SENT16 = 0x7FC0BEEF, 0x7FBE  # NaN payloads: no sum has these bits
TAIL = 128


def stream():
    return torch.cuda.current_stream().cuda_stream


def sentinels(n):
    """(int32, int16) device buffers of n + TAIL sentinels: an out_f32 and an out_dt."""
    return (torch.full((n + TAIL,), SENT32, dtype=torch.int32, device="cuda"),
            torch.full((n + TAIL,), SENT16, dtype=torch.int16, device="cuda"))


@pytest.mark.parametrize("L, ql", [(130, 70), (128, 128)])
def test_padded_rows_both_outputs_and_nothing_between_them(L, ql):
    B, G, D, stride = 2, 3, 128, L + 5
    k, q = randn_inputs(50, BF16, B, G, L, ql, D)
    rows = B * HKV * G
    o32, o16 = sentinels(rows * stride)
    t = table([k], [q], None, [o32], [o16], [stride])
    p = params(k, q)
    rc, nbytes = N.colsum_plan(p, t)
    assert rc == 0 and nbytes == scratch_bytes(rows, ql, L)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert N.colsum_score(p, t, scratch.data_ptr(), nbytes, stream()) == 0
    torch.cuda.synchronize()
    f32 = o32.view(torch.float32)[:rows * stride].view(B, HKV * G, stride)
    err = rel_err(f32[..., :L], reference(k, q)[0])
    print(f"colsum out_stride = L + 5, ({L}, {ql}): max relative error {err:.3e}")
    assert err < BOUND
    d16 = o16.view(BF16)[:rows * stride].view(B, HKV * G, stride)
    assert torch.equal(d16[..., :L], f32[..., :L].to(BF16))
    for buf, sent in ((o32, SENT32), (o16, SENT16)):
        assert (buf[:rows * stride].view(rows, stride)[:, L:] == sent).all(), "a write into a gap"
        assert (buf[rows * stride:] == sent).all(), "a write past the last row"


def test_exact_scratch_is_enough_and_nothing_around_it_is_touched():
    B, G, D, L, ql = 2, 3, 128, 1100, 48  # mb = 2, three key splits
    k, q = randn_inputs(51, BF16, B, G, L, ql, D)
    rows = B * HKV * G
    want = attention_column_sums(k, q)
    o32, _ = sentinels(rows * L)
    t = table([k], [q], None, [o32])
    p = params(k, q)
    rc, nbytes = N.colsum_plan(p, t)
    assert rc == 0 and nbytes == scratch_bytes(rows, ql, L)
    buf = torch.full((256 + nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = buf.data_ptr() + 256
    assert ptr % 16 == 0

    # colsum_score_impl refuses these after the plan's checks and before its first launch
    assert N.colsum_score(p, t, ptr, nbytes - 1, stream()) == E_WORKSPACE
    assert N.colsum_score(p, t, 0, nbytes, stream()) == E_WORKSPACE
    assert N.colsum_score(p, t, ptr + 4, nbytes, stream()) == E_ALIGN
    assert N.colsum_score(p, t[:0], ptr, nbytes, stream()) == 0  # no layers: KVC_OK, nothing runs
    torch.cuda.synchronize()
    assert (o32 == SENT32).all() and (buf == 0xA5).all()

    assert N.colsum_score(p, t, ptr, nbytes, stream()) == 0
    torch.cuda.synchronize()
    assert (buf[:256] == 0xA5).all(), "a write before the scratch"
    assert (buf[256 + nbytes:] == 0xA5).all(), "a write past the scratch"
    assert torch.equal(o32.view(torch.float32)[:rows * L].view(B, HKV * G, L), want)
    assert (o32[rows * L:] == SENT32).all()


def test_a_callers_lse_needs_no_scratch_at_all():
    k, q = randn_inputs(52, BF16, 2, 3, 130, 70, 128)
    lse = reference(k, q)[1].float().cuda()
    rows = 2 * HKV * 3
    o32, _ = sentinels(rows * 130)
    t = table([k], [q], [lse], [o32])
    p = params(k, q)
    assert N.colsum_plan(p, t) == (0, 0)
    assert N.colsum_score(p, t, 0, 0, stream()) == 0  # scratch may be NULL
    torch.cuda.synchronize()
    assert torch.equal(o32.view(torch.float32)[:rows * 130].view(2, HKV * 3, 130),
                       attention_column_sums(k, q, lse=lse))
    assert (o32[rows * 130:] == SENT32).all()
