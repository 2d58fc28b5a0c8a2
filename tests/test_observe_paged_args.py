"""kvc_observe_plan_paged (a pure host function: no GPU) accepts dense tables as kvc_observe_plan
does, fp8 keys and page tables, and refuses what include/kvc.h's "Paged and fp8 keys" rules out,
each with its status code."""
import numpy as np
import pytest

from kvcompress import _native as N

E_ARG, E_DTYPE, E_ALIGN = -1, -2, -4
F8 = (N.KVC_F8E4M3, N.KVC_F8E5M2)


def _plan(dtype=N.KVC_BF16, H=2, D=128, S=300, W=32, P=None, table=4096, cols=None, layer=(),
          page=()):
    """(rc, scratch bytes, kvc_observe_plan's (rc, bytes)) on a one-layer table as kvc_plan leaves
    it: dense [1, H, S, D] K, or with P a pool stored [N, H, P, D] behind a one-row table."""
    t = np.zeros(1, dtype=N.LAYER_DTYPE)
    t["k"] = t["v"] = t["k_out"] = t["v_out"] = 4096
    t["k_stride"] = t["v_stride"] = (H * S * D, S * D, D) if P is None else (0, P * D, D)
    t["seq_len"], t["zone_len"], t["n_select"] = S, S - W, 8
    t["tail_start"], t["tail_len"] = S - W, W
    for name, v in layer:
        t[name] = v
    p = N.Params(dtype=dtype, batch=1, heads=H, head_dim=D, order=N.KVC_DESC,
                 algo=N.KVC_ALGO_TOPK, phases=N.PHASE_ALL)
    N.plan(p, t)
    o = np.zeros(1, dtype=N.OBSERVE_LAYER_DTYPE)
    o["q"], o["q_stride"] = 8192, (H * W * D, W * D, D)
    op = N.ObserveParams(q_heads=H, window=W, scale=0.0, pool_kernel=5, pool_mode=0)
    pages = None
    if P is not None:
        pages = np.zeros(1, dtype=N.PAGES_DTYPE)
        pages[0] = (table, -(-S // P) if cols is None else cols, H * P * D, H * P * D, P, 64, 1, 0)
        for name, v in page:
            pages[name] = v
    return N.observe_plan_paged(p, op, t, o, pages) + (N.observe_plan(p, op, t, o),)


@pytest.mark.parametrize("kw", [
    dict(), dict(dtype=N.KVC_F16, D=64, W=16), dict(D=256, S=5000),
    *[dict(dtype=dt, D=D) for dt in F8 for D in (64, 128, 256)],
    dict(P=1), dict(P=16), dict(P=4096), dict(P=16, dtype=N.KVC_F8E4M3, D=64),
    dict(P=16, page=[("in_place", 7)]),  # not read
])
def test_accepts(kw):
    rc, nbytes, dense = _plan(**kw)
    assert rc == 0 and nbytes > 0 and nbytes % 4 == 0
    if "P" not in kw and kw.get("dtype") not in F8:
        assert dense == (0, nbytes)  # what kvc_observe_plan accepts, with equal scratch bytes
    elif kw.get("dtype") in F8:
        assert dense[0] == E_DTYPE  # the dense pair keeps its rule set


@pytest.mark.parametrize("kw, code", [
    (dict(P=16, layer=[("k_stride", (2048, 2048, 128))]), E_ARG),  # the table is the batch dim
    (dict(P=24), E_ARG), (dict(P=0, cols=300), E_ARG),
    (dict(P=16, cols=18), E_ARG),  # ceil(300 / 16) = 19
    (dict(P=16, table=0), E_ARG), (dict(P=16, table=4098), E_ARG),
    (dict(P=16, page=[("num_pages", 0)]), E_ARG), (dict(P=16, page=[("reserved", 1)]), E_ARG),
    (dict(P=16, page=[("k_page_stride", 4100)]), E_ALIGN),
    (dict(dtype=N.KVC_F8E4M3, D=64, layer=[("k_stride", (38400, 19200, 72))]), E_ALIGN),
    (dict(dtype=N.KVC_F8E5M2, P=16, layer=[("k_stride", (0, 2056, 128))]), E_ALIGN),
    (dict(dtype=N.KVC_F32), E_DTYPE), (dict(dtype=N.KVC_F32, P=16), E_DTYPE),
])
def test_refuses(kw, code):
    assert _plan(**kw)[0] == code
