"""Argument errors of the `out` kwarg that need no device: every check here precedes the engine's
own device check, so CPU (and meta) tensors reach it.  Nothing is enqueued -- there is no GPU."""
import pytest
import torch

from kvcompress.methods import (fix_size_l2_compress, get_compress_fn, list_methods,
                                recent_only_compress, streaming_llm_compress)
from kvcompress.methods.streaming_llm import evict_for_space

B, H, S, D = 2, 3, 600, 64
KW = dict(fix_kv_size=100, keep_ratio=0.25, skip_layers=[])


def _kv(dtype=torch.bfloat16, n=1):
    return [(torch.zeros(B, H, S, D, dtype=dtype), torch.zeros(B, H, S, D, dtype=dtype))
            for _ in range(n)]


def _dst(shape=(B, H, 128, D), dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype), torch.zeros(shape, dtype=dtype)


def test_every_compress_function_takes_out():
    """out=None is the default call; anything but None / "inplace" / a list is refused by the
    nine registered methods and evict_for_space alike (before the layers are looked at)."""
    fns = [get_compress_fn(m) for m in list_methods()] + [evict_for_space]
    assert len(fns) == 10
    for fn in fns:
        extra = dict(num_coming=1) if fn is evict_for_space else {}
        assert fn([], out=None, **extra) == []
        with pytest.raises(TypeError, match="out must be"):
            fn(_kv(), out=3, **extra)
        with pytest.raises(ValueError, match="inplace"):
            fn(_kv(), out="in-place", **extra)
        with pytest.raises(ValueError, match="2 entries for 1 layers"):
            fn(_kv(), out=[None, None], **extra)
        with pytest.raises(TypeError, match="layer 0"):
            fn(_kv(), out=[torch.zeros(1)], **extra)


def test_out_none_entries_keep_the_default_behaviour():
    kv = _kv()
    out = recent_only_compress(kv, window_size=50, skip_layers=[], out=[None])
    assert out[0][0].data_ptr() == kv[0][0][:, :, -50:].data_ptr() and out[0][0].shape[2] == 50


@pytest.mark.parametrize("which", [0, 1])
def test_destination_dtype_shape_and_strides(which):
    def call(kd, vd):
        return fix_size_l2_compress(_kv(n=2), out=[None, (kd, vd)], **KW)

    def swap(good, bad):
        return (bad, good) if which == 0 else (good, bad)

    good = _dst()[0]
    with pytest.raises(TypeError, match="layer 1.*dtype"):
        call(*swap(good, _dst(dtype=torch.float16)[0]))
    for shape in ((B + 1, H, 128, D), (B, H + 1, 128, D), (B, H, 128, D + 16), (B, H, 128)):
        with pytest.raises(ValueError, match="layer 1.*destination must be"):
            call(*swap(good, torch.zeros(shape, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="layer 1.*last dim"):
        call(*swap(good, torch.zeros(B, H, D, 128, dtype=torch.bfloat16).transpose(2, 3)))
    with pytest.raises(ValueError, match="layer 1.*16"):  # seq stride of 68 elements = 136 bytes
        call(*swap(good, torch.zeros(B, H, 128, D + 4, dtype=torch.bfloat16)[..., :D]))
    with pytest.raises(ValueError, match="layer 1.*16"):  # pointer 8 bytes off
        call(*swap(good, torch.zeros(B, H, 128, D + 8, dtype=torch.bfloat16)[..., 4:4 + D]))
    with pytest.raises(ValueError, match="layer 1.* is on meta"):
        call(*swap(good, torch.zeros(B, H, 128, D, dtype=torch.bfloat16, device="meta")))
    with pytest.raises(TypeError, match="layer 1.*must be a tensor"):
        call(*swap(good, None))


def test_inplace_refuses_inputs_the_engine_would_copy():
    k, v = _kv()[0]
    padded = torch.zeros(B, H, S, D + 4, dtype=torch.bfloat16)[..., :D]  # 136-byte rows
    off = torch.zeros(B, H, S, D + 8, dtype=torch.bfloat16)[..., 4:4 + D]  # pointer 8 bytes off
    lastdim = torch.zeros(B, H, D, S, dtype=torch.bfloat16).transpose(2, 3)
    for bad in (padded, off, lastdim):
        with pytest.raises(ValueError, match="layer 0: K cannot be compacted in place.*copy"):
            fix_size_l2_compress([(bad, v)], out="inplace", **KW)
        with pytest.raises(ValueError, match="layer 0: V cannot be compacted in place.*copy"):
            fix_size_l2_compress([(k, bad)], out="inplace", **KW)


def test_inplace_refuses_zero_strides_and_shared_memory():
    k, v = _kv()[0]
    exp = torch.zeros(1, H, S, D, dtype=torch.bfloat16).expand(B, H, S, D)
    with pytest.raises(ValueError, match="layer 0: K.*stride 0"):
        fix_size_l2_compress([(exp, v)], out="inplace", **KW)
    with pytest.raises(ValueError, match="layer 0: V.*stride 0"):
        fix_size_l2_compress([(k, exp)], out="inplace", **KW)
    with pytest.raises(ValueError, match="layer 0: V shares its memory with layer 0's K"):
        fix_size_l2_compress([(k, k)], out="inplace", **KW)
    with pytest.raises(ValueError, match="layer 1: K shares its memory with layer 0's V"):
        fix_size_l2_compress([(k, v), (v, torch.zeros_like(v))], out="inplace", **KW)


def test_inplace_refuses_unordered_segments():
    """streaming_llm(recent_size=0) keeps the reference's `-0:` quirk: the sinks and then the
    whole sequence, a result longer than its input."""
    with pytest.raises(ValueError, match="layer 0: cannot be compacted in place.*recent_size=0"):
        streaming_llm_compress(_kv(), start_size=4, recent_size=0, out="inplace")


def test_short_and_overlapping_destinations():
    kv = _kv()
    short = _dst((B, H, 99, D))
    with pytest.raises(ValueError, match="layer 0: K destination holds 99 rows, the result has 100"):
        fix_size_l2_compress(kv, out=[short], **KW)
    cache = torch.zeros(2, B, H, S + 200, D, dtype=torch.bfloat16)
    k, v = cache[0][:, :, :S], cache[1][:, :, :S]
    other = _dst()[0]
    with pytest.raises(ValueError, match="layer 0: K destination overlaps the layer's K"):
        fix_size_l2_compress([(k, v)], out=[(cache[0][:, :, S:], other)], **KW)
    with pytest.raises(ValueError, match="layer 0: V destination overlaps the layer's K"):
        fix_size_l2_compress([(k, v)], out=[(other, cache[0][:, :, S:])], **KW)


def test_a_passed_through_layer_is_checked_before_the_other_layers_launch():
    """Layer 1 is skipped by the method, so its destination is only filled by a copy after the
    method ran; its too-short (or overlapping) destination must still be refused together with
    layer 0's job, before anything launches.  On CPU tensors a launch attempt would raise the
    engine's RuntimeError (no CPU path) instead of these ValueErrors."""
    kv = _kv(n=2)
    kw = dict(fix_kv_size=100, keep_ratio=0.25, skip_layers=[1])
    for first in ("inplace", _dst()):
        with pytest.raises(ValueError, match="layer 1: K destination holds 99 rows, the result has 600"):
            fix_size_l2_compress(kv, out=[first, _dst((B, H, 99, D))], **kw)
    cache = torch.zeros(B, H, 2 * S, D, dtype=torch.bfloat16)
    k1 = cache[:, :, :S]
    with pytest.raises(ValueError, match="layer 1: K destination overlaps the layer's K"):
        fix_size_l2_compress([kv[0], (k1, kv[1][1])],
                             out=["inplace", (cache[:, :, 100:100 + S], _dst((B, H, S, D))[1])], **kw)
    # a sliced layer (recent_only) likewise
    with pytest.raises(ValueError, match="layer 0: V destination holds 49 rows, the result has 50"):
        recent_only_compress(_kv(), window_size=50, skip_layers=[],
                             out=[(_dst()[0], _dst((B, H, 49, D))[1])])
