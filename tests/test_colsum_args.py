"""kvc_colsum_plan (a pure host function: no GPU) refuses what include/kvc.h's "Causal attention
column sums" section rules out, each with its status code, and reports the documented scratch;
the Python entry points refuse CPU, fp8 and mixed layer groups before anything launches."""
import numpy as np
import pytest
import torch

from kvcompress import _native as N
from kvcompress import attention_column_sums
from kvcompress.methods.h2o_attention import H2OAttentionManager

E_ARG, E_DTYPE, E_HEADDIM, E_ALIGN = -1, -2, -3, -4


def _plan(dtype=N.KVC_BF16, B=1, H=2, D=128, L=300, q=40, G=1, layer=(), **params):
    """(rc, scratch bytes) of kvc_colsum_plan on a one-layer table of dense K and Q."""
    t = np.zeros(1, dtype=N.COLSUM_LAYER_DTYPE)
    t["k"], t["q"], t["out_f32"], t["out_dt"] = 4096, 8192, 12288, 16384
    t["k_stride"], t["q_stride"] = (H * L * D, L * D, D), (G * H * q * D, q * D, D)
    t["out_stride"], t["seq_len"], t["q_len"] = L, L, q
    for name, v in layer:
        t[name] = v
    kw = dict(dtype=dtype, batch=B, heads=H, q_heads=G * H, head_dim=D, scale=0.0)
    kw.update(params)
    return N.colsum_plan(N.ColsumParams(**kw), t)


@pytest.mark.parametrize("kw, code", [
    (dict(dtype=N.KVC_F32), E_DTYPE), (dict(dtype=N.KVC_F8E4M3), E_DTYPE),
    (dict(dtype=N.KVC_F8E5M2), E_DTYPE),
    (dict(D=32), E_HEADDIM), (dict(D=96), E_HEADDIM), (dict(D=512), E_HEADDIM),
    (dict(G=17), E_ARG), (dict(q_heads=3), E_ARG), (dict(q_heads=1), E_ARG),
    (dict(q=301), E_ARG), (dict(q=0), E_ARG), (dict(L=(1 << 20) + 1), E_ARG),
    (dict(scale=float("inf")), E_ARG), (dict(reserved=(0, 1)), E_ARG),
    (dict(layer=[("reserved", 1)]), E_ARG), (dict(layer=[("out_stride", 299)]), E_ARG),
    (dict(layer=[("q", 0)]), E_ARG), (dict(layer=[("out_f32", 0), ("out_dt", 0)]), E_ARG),
    (dict(layer=[("k", 4104)]), E_ALIGN), (dict(layer=[("lse", 4098)]), E_ALIGN),
    (dict(layer=[("out_dt", 16385)]), E_ALIGN),
    (dict(layer=[("q_stride", (10240, 5124, 128))]), E_ALIGN),
    (dict(layer=[("k_stride", (76800, 38400, 132))]), E_ALIGN),
])
def test_colsum_plan_refuses(kw, code):
    assert _plan(**kw)[0] == code


def scratch_formula(R, q, L):
    """include/kvc.h: lse rows + (max, sum) partials of one layer without lse."""
    mb = 1 if q <= 32 else 2 if q <= 64 else 4
    nqb, tiles = -(-q // (32 * mb)), -(-L // 128)
    want = min(max(-(-1024 // (R * nqb)), 1), min(32, -(-tiles // 4)))
    tps = -(-tiles // want)
    return -(-4 * R * q // 256) * 256 + 1024 * R * nqb * -(-tiles // tps)


@pytest.mark.parametrize("kw", [
    dict(), dict(dtype=N.KVC_F16, D=64, G=16, q=1), dict(D=80, q=300), dict(D=256, B=3, G=3),
    dict(L=16384, q=64, H=8), dict(L=1 << 20, q=1 << 20, layer=[("out_dt", 0)]),
])
def test_colsum_plan_accepts_and_sizes_scratch(kw):
    rc, nbytes = _plan(**kw)
    R = kw.get("B", 1) * kw.get("H", 2) * kw.get("G", 1)
    assert rc == 0 and nbytes == scratch_formula(R, kw.get("q", 40), kw.get("L", 300))
    with_lse = {**kw, "layer": list(kw.get("layer", ())) + [("lse", 4096)]}
    assert _plan(**with_lse) == (0, 0)  # a caller's lse: no statistics, no scratch


def test_python_refusals_before_any_launch():
    k, q = torch.zeros(1, 2, 40, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 8, 64, dtype=torch.bfloat16)
    mgr = H2OAttentionManager()
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        attention_column_sums(k, q)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        mgr.update_from_queries([q], [(k, k)])
    for bad in (torch.float8_e4m3fn, torch.float32):
        with pytest.raises(TypeError, match="bfloat16 or float16"):
            attention_column_sums(k.to(bad), q.to(bad))
        with pytest.raises(TypeError, match="bfloat16 or float16"):
            mgr.update_from_queries([q.to(bad)], [k.to(bad)])
    with pytest.raises(ValueError, match="share B, Hkv, Hq, D"):
        attention_column_sums([k, k[:, :1]], [q, q[:, :1]])
    with pytest.raises(ValueError, match="queries must be"):
        attention_column_sums(k[:, :, :4], q)  # q > L
    assert mgr.accumulated_attention == {} and mgr.current_seq_len == 0
