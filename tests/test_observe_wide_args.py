"""kvc_observe_plan_paged (a pure host function: no GPU) admits every group size G <= 16 with
G * window <= 256 (include/kvc.h, "Wide query groups") and still refuses what lies past that."""
import numpy as np
import pytest

from kvcompress import _native as N

E_ARG = -1


def _plan(G, W, dtype=N.KVC_BF16, H=2, D=128, S=300, P=None):
    """(rc, scratch bytes) on a one-layer table as kvc_plan leaves it: dense [1, H, S, D] K, or
    with P a pool stored [N, H, P, D] behind a one-row table."""
    t = np.zeros(1, dtype=N.LAYER_DTYPE)
    t["k"] = t["v"] = t["k_out"] = t["v_out"] = 4096
    t["k_stride"] = t["v_stride"] = (H * S * D, S * D, D) if P is None else (0, P * D, D)
    t["seq_len"], t["zone_len"], t["n_select"] = S, S - W, 8
    t["tail_start"], t["tail_len"] = S - W, W
    p = N.Params(dtype=dtype, batch=1, heads=H, head_dim=D, order=N.KVC_DESC,
                 algo=N.KVC_ALGO_TOPK, phases=N.PHASE_ALL)
    N.plan(p, t)
    o = np.zeros(1, dtype=N.OBSERVE_LAYER_DTYPE)
    o["q"], o["q_stride"] = 8192, (G * H * W * D, W * D, D)
    op = N.ObserveParams(q_heads=G * H, window=W, scale=0.0, pool_kernel=5, pool_mode=0)
    pages = None
    if P is not None:
        pages = np.zeros(1, dtype=N.PAGES_DTYPE)
        pages[0] = (4096, -(-S // P), H * P * D, H * P * D, P, 64, 1, 0)
    return N.observe_plan_paged(p, op, t, o, pages)


@pytest.mark.parametrize("G, W, kw", [
    (3, 16, dict(D=64)), (3, 32, dict()), (5, 16, dict(dtype=N.KVC_F16)), (5, 32, dict(S=5000)),
    (6, 32, dict(P=16)), (7, 32, dict(dtype=N.KVC_F8E4M3)), (8, 32, dict()),
    (8, 32, dict(dtype=N.KVC_F8E5M2, P=256, D=64)), (4, 64, dict(D=256)), (16, 16, dict(D=256)),
])
def test_accepts_wide_groups(G, W, kw):
    rc, nbytes = _plan(G, W, **kw)
    assert rc == 0 and nbytes > 0 and nbytes % 4 == 0


@pytest.mark.parametrize("G, W", [(17, 16), (8, 64), (16, 32)])
def test_refuses_past_the_limit(G, W):
    assert _plan(G, W)[0] == E_ARG
