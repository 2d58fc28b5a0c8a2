"""kvc_observe_plan (a pure host function: no GPU) refuses what include/kvc.h's "Observation-window
scores" section rules out, each with its status code, and sizes its scratch monotonically in S."""
import numpy as np
import pytest

from kvcompress import _native as N

E_ARG, E_DTYPE, E_HEADDIM, E_ALIGN = -1, -2, -3, -4


def _plan(dtype=N.KVC_BF16, B=1, H=2, D=128, S=300, W=32, G=1, zone=None, k=8, pool=5, mode=0,
          layer=(), olayer=(), op=(), **params):
    """(rc, scratch bytes) of kvc_observe_plan on a one-layer table as kvc_plan leaves it."""
    z0, zl = zone if zone is not None else (0, S - W)
    t = np.zeros(1, dtype=N.LAYER_DTYPE)
    t["k"] = t["v"] = t["k_out"] = t["v_out"] = 4096
    t["k_stride"] = t["v_stride"] = (H * S * D, S * D, D)
    t["seq_len"], t["zone_start"], t["zone_len"], t["n_select"] = S, z0, zl, min(k, zl)
    t["tail_start"], t["tail_len"] = S - W, W
    for name, v in layer:
        t[name] = v
    p = N.Params(dtype=dtype, batch=B, heads=H, head_dim=D, order=N.KVC_DESC,
                 algo=N.KVC_ALGO_TOPK, phases=N.PHASE_ALL, **params)
    N.plan(p, t)  # fills the planned fields (what it refuses itself, kvc_observe_plan refuses too)
    o = np.zeros(1, dtype=N.OBSERVE_LAYER_DTYPE)
    o["q"], o["q_stride"] = 8192, (G * H * W * D, W * D, D)
    for name, v in olayer:
        o[name] = v
    kw = dict(q_heads=G * H, window=W, scale=0.0, pool_kernel=pool, pool_mode=mode)
    kw.update(op)
    return N.observe_plan(p, N.ObserveParams(**kw), t, o)


@pytest.mark.parametrize("kw, code", [
    (dict(dtype=N.KVC_F32), E_DTYPE), (dict(dtype=N.KVC_F8E4M3), E_DTYPE),
    (dict(dtype=N.KVC_F8E5M2, D=64), E_DTYPE),
    (dict(D=32), E_HEADDIM), (dict(D=80), E_HEADDIM),
    (dict(W=8), E_ARG), (dict(W=48), E_ARG), (dict(W=128, S=400), E_ARG),
    (dict(G=3), E_ARG), (dict(G=16, W=16), E_ARG), (dict(G=4, W=64), E_ARG),
    (dict(op=dict(q_heads=3)), E_ARG),
    (dict(pool=4), E_ARG), (dict(pool=9), E_ARG), (dict(pool=0), E_ARG), (dict(mode=2), E_ARG),
    (dict(op=dict(reserved=1)), E_ARG), (dict(op=dict(scale=float("nan"))), E_ARG),
    (dict(S=32, zone=(0, 0), layer=[("zone_len", 1), ("n_select", 1)]), E_ARG),  # S < W + 1
    (dict(zone=(0, 269)), E_ARG), (dict(zone=(200, 100)), E_ARG),  # past S - W
    (dict(layer=[("score_mode", N.KVC_SCORE_SNAPKV)]), E_ARG),
    (dict(external_index=1), E_ARG),
    (dict(olayer=[("q", 0)]), E_ARG), (dict(olayer=[("reserved", 1)]), E_ARG),
    (dict(olayer=[("q", 8200)]), E_ALIGN), (dict(olayer=[("q_stride", (8192, 4100, 128))]), E_ALIGN),
    (dict(olayer=[("q_stride", (8192, 4096, 132))]), E_ALIGN),
    (dict(layer=[("k_stride", (76800, 38400, 132))]), E_ALIGN),
])
def test_observe_plan_refuses(kw, code):
    assert _plan(**kw)[0] == code


@pytest.mark.parametrize("kw", [
    dict(), dict(dtype=N.KVC_F16, D=64, W=16, G=8), dict(D=256, W=64, G=2), dict(G=4),
    dict(S=33, k=0, zone=(0, 1)), dict(pool=7, mode=1, zone=(5, 3)), dict(zone=(0, 0), k=0),
    dict(op=dict(scale=0.25)),
])
def test_observe_plan_accepts(kw):
    rc, nbytes = _plan(**kw)
    assert rc == 0 and nbytes % 4 == 0


def test_scratch_grows_with_the_sequence():
    sizes = [_plan(S=S)[1] for S in (33, 64, 1000, 1024, 1025, 1056, 1057, 5000, 20000)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0]
    assert _plan(S=5000, B=2)[1] >= 2 * _plan(S=5000)[1] - 512  # rows scale it (256-B rounding)
