"""kvc_plan_paged's host-side contract (include/kvc.h, "Paged caches"): every validation rule
gives its stated code, pages = NULL is kvc_plan_dest, and a page table never changes what kvc_plan
fills in.  CPU only: kvc_plan_paged is a pure host function (no pointer is dereferenced)."""
import os
import re

import numpy as np
import pytest

import test_abi
from kvcompress import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_ALIGN = -1, -4
B, H, D, ES = 2, 3, 64, 2
S, P, NPAGES = 1000, 16, 2 * 63 + 7
POOL_K, POOL_V = 4 << 20, 8 << 20      # two pools of NPAGES pages (about 400 KiB each)
DST_K, DST_V = 16 << 20, 24 << 20
TABLE = 1 << 20
NHPD = (P * D, D)                      # head / slot strides of a pool stored [N, H, P, D]
NPHD = (D, H * D)                      # ... stored [N, P, H, D]
PAGE = H * P * D                       # page stride of both


def _params(**kw):
    d = dict(dtype=N.KVC_BF16, batch=B, heads=H, head_dim=D, order=0, algo=0, phases=N.PHASE_ALL,
             external_index=0)
    d.update(kw)
    return N.Params(**d)


def _layer(inplace, sink=4, zs=4, zl=700, k=100, ts=704, tl=296, **kw):
    t = np.zeros(1, dtype=N.LAYER_DTYPE)[0]
    t["k"], t["v"] = POOL_K, POOL_V
    t["k_out"], t["v_out"] = (POOL_K, POOL_V) if inplace else (DST_K, DST_V)
    t["k_stride"], t["v_stride"] = (0,) + NHPD, (0,) + NPHD
    t["seq_len"], t["zone_start"], t["zone_len"], t["n_select"] = S, zs, zl, k
    t["sink_len"], t["tail_start"], t["tail_len"] = sink, ts, tl
    for name, val in kw.items():
        t[name] = val
    return t


def _pages(inplace, **kw):
    g = np.zeros(1, dtype=N.PAGES_DTYPE)[0]
    g["block_table"], g["table_stride"] = TABLE, 63
    g["k_page_stride"] = g["v_page_stride"] = PAGE
    g["page_size"], g["num_pages"], g["in_place"] = P, NPAGES, int(inplace)
    for name, val in kw.items():
        g[name] = val
    return g


def _dest(**kw):
    d = np.zeros(1, dtype=N.DEST_DTYPE)[0]
    n = 400
    d["k_stride"] = d["v_stride"] = (H * n * D, n * D, D)
    for name, val in kw.items():
        d[name] = val
    return d


def _plan(layer, pages, dest=None, **pkw):
    table = np.array([layer], dtype=N.LAYER_DTYPE)
    rc, info = N.plan_paged(_params(**pkw), table, np.array([pages], dtype=N.PAGES_DTYPE),
                            None if dest is None else np.array([dest], dtype=N.DEST_DTYPE))
    return rc


def _info(i):
    return tuple(getattr(i, f) for f, _ in N.PlanInfo._fields_)


def test_struct_size_and_declarations():
    assert N.PAGES_DTYPE.itemsize == 48
    assert {"kvc_plan_paged", "kvc_launch_paged"} <= set(N.EXPORTS)
    assert {"kvc_plan_paged", "kvc_launch_paged"} <= set(test_abi._declared_functions())
    # the declaration scan sees lowercase names only: the header gained no function-like macro
    assert all(re.fullmatch(r"kvc_[a-z_]+", n) for n in test_abi._declared_functions())
    hdr = open(os.path.join(ROOT, "include", "kvc.h")).read()
    assert "} kvc_pages_t;" in hdr
    assert N.lib().kvc_version() == 4 and N.lib().kvc_layer_struct_size() == 136
    assert hasattr(N.lib(), "kvc_plan_paged") and hasattr(N.lib(), "kvc_launch_paged")


def test_pages_null_is_kvc_plan_dest():
    import test_dest_plan as DP
    for inplace in (False, True):
        t0 = np.array([DP._layer(inplace)], dtype=N.LAYER_DTYPE)
        t1 = t0.copy()
        dests = np.array([DP._dest(inplace)], dtype=N.DEST_DTYPE)
        rc0, i0 = N.plan_dest(DP._params(), t0, dests)
        rc1, i1 = N.plan_paged(DP._params(), t1, None, dests)
        assert rc0 == rc1 == 0 and _info(i0) == _info(i1) and t0.tobytes() == t1.tobytes()
        dests[0]["reserved"] = 1
        assert N.plan_paged(DP._params(), t1, None, dests)[0] == E_ARG
        assert N.launch_paged(DP._params(), t1, None, dests, None, 0, None) == E_ARG
    t = np.array([DP._layer(False)], dtype=N.LAYER_DTYPE)
    rc0, i0 = N.plan(DP._params(), t.copy())
    rc1, i1 = N.plan_paged(DP._params(), t, None, None)
    assert rc0 == rc1 == 0 and _info(i0) == _info(i1)


def test_valid_tables_plan_like_kvc_plan():
    """The three output modes fill the same layer fields and kvc_plan_info_t as kvc_plan."""
    def table(inplace):
        return np.array([_layer(inplace), _layer(inplace, zl=600, k=600, ts=700, tl=300),
                         _layer(inplace, sink=4, zs=0, zl=0, k=0, ts=500, tl=500)],
                        dtype=N.LAYER_DTYPE)
    want = table(False)
    rc, winfo = N.plan(_params(), want)
    assert rc == 0
    for inplace, dests in ((False, None), (False, np.array([_dest()] * 3, dtype=N.DEST_DTYPE)),
                           (True, None)):
        t = table(inplace)
        pages = np.array([_pages(inplace)] * 3, dtype=N.PAGES_DTYPE)
        rc, info = N.plan_paged(_params(), t, pages, dests)
        assert rc == 0, (inplace, dests is None)
        assert _info(info) == _info(winfo)
        for f in ("n_out", "row0", "tile0", "unit0"):
            assert list(t[f]) == list(want[f]), (inplace, f)
        # launch re-validates before it touches the device; the workspace check comes after
        bad = pages.copy()
        bad[1]["reserved"] = 1
        assert N.launch_paged(_params(), t, bad, dests, None, 0, None) == E_ARG
        assert N.launch_paged(_params(), t, pages, dests, None, 0, None) == -6  # KVC_E_WORKSPACE


@pytest.mark.parametrize("inplace", [False, True])
def test_page_description_refusals(inplace):
    ok = _layer(inplace)
    assert _plan(ok, _pages(inplace)) == 0
    for kw in (dict(block_table=0), dict(block_table=TABLE + 2), dict(table_stride=62),
               dict(page_size=0), dict(page_size=24), dict(page_size=-16),
               dict(page_size=131072, table_stride=63), dict(num_pages=0), dict(num_pages=-1),
               dict(in_place=2), dict(in_place=-1), dict(reserved=1)):
        assert _plan(ok, _pages(inplace, **kw)) == E_ARG, kw
    assert _plan(ok, _pages(inplace, table_stride=63)) == 0           # ceil(1000 / 16)
    assert _plan(ok, _pages(inplace, table_stride=1000)) == 0          # larger than needed
    assert _plan(ok, _pages(inplace, page_size=65536, table_stride=1)) == 0
    assert _plan(ok, _pages(inplace, page_size=1, table_stride=1000)) == 0
    # the table replaces the batch stride
    assert _plan(_layer(inplace, k_stride=(PAGE,) + NHPD), _pages(inplace)) == E_ARG
    assert _plan(_layer(inplace, v_stride=(PAGE,) + NPHD), _pages(inplace)) == E_ARG
    # a layer without output is exempt
    empty = _layer(inplace, sink=0, zs=0, zl=0, k=0, ts=0, tl=0)
    assert _plan(empty, _pages(inplace, reserved=7, page_size=3)) == 0


@pytest.mark.parametrize("side", ["k", "v"])
def test_alignment_rules(side):
    """The inputs' rules: head and slot strides as for dense inputs; the page stride counts as a
    dim larger than 1 when num_pages > 1."""
    st = {"k": (0,) + NHPD, "v": (0,) + NPHD}[side]
    for dim in (1, 2):
        bad = list(st)
        bad[dim] += 4  # 8 bytes off
        assert _plan(_layer(False, **{side + "_stride": tuple(bad)}), _pages(False)) == E_ALIGN
    assert _plan(_layer(False), _pages(False, **{side + "_page_stride": PAGE + 4})) == E_ALIGN
    assert _plan(_layer(False), _pages(False, num_pages=1,
                                       **{side + "_page_stride": PAGE + 4})) == 0
    lay = _layer(False)
    lay[side] += 8  # the pool base
    assert _plan(lay, _pages(False)) == E_ALIGN


def test_in_place_rules():
    ok = _layer(True)
    assert _plan(ok, _pages(True)) == 0
    assert _plan(_layer(True, k_out=DST_K), _pages(True)) == E_ARG
    assert _plan(_layer(True, v_out=DST_V), _pages(True)) == E_ARG
    # dests[i] is not read in place
    assert _plan(ok, _pages(True), _dest(reserved=9, in_place=5)) == 0
    # the segment-order rules of kvc_dest_t's in-place contract
    cases = [
        (dict(sink=8, zs=4), E_ARG),
        (dict(sink=0, zs=0, zl=800, k=100, ts=700), E_ARG),
        (dict(sink=4, zs=0, zl=0, k=0, ts=0, tl=1000), E_ARG),  # streaming_llm(recent_size=0)
        (dict(sink=8, zs=4, k=0), 0),
        (dict(sink=4, zs=4, zl=700, k=100, ts=0, tl=0), 0),
        (dict(sink=0, zs=0, zl=1000, k=900, ts=0, tl=0), 0),
    ]
    for kw, code in cases:
        assert _plan(_layer(True, **kw), _pages(True)) == code, kw
        assert _plan(_layer(False, **kw), _pages(False)) == 0, kw
    # zero strides would make different rows one address
    assert _plan(_layer(True, k_stride=(0, 0, D)), _pages(True)) == E_ARG
    assert _plan(_layer(True, v_stride=(0, D, 0)), _pages(True)) == E_ARG
    assert _plan(ok, _pages(True, k_page_stride=0)) == E_ARG
    assert _plan(_layer(False, k_stride=(0, 0, D)), _pages(False)) == 0  # fine as a source


def test_dense_destination_rules():
    ok = _layer(False)
    assert _plan(ok, _pages(False), _dest()) == 0
    assert _plan(ok, _pages(False), _dest(in_place=1)) == E_ARG
    assert _plan(ok, _pages(False), _dest(reserved=1)) == E_ARG
    n = 400
    for dim in (0, 1, 2):
        st = [H * n * D, n * D, D]
        st[dim] += 4
        assert _plan(ok, _pages(False), _dest(k_stride=tuple(st))) == E_ALIGN
        assert _plan(ok, _pages(False), _dest(v_stride=tuple(st))) == E_ALIGN
    # the destination's span must not meet a pool's span: NPAGES pages from the base
    pool_bytes = ((NPAGES - 1) * PAGE + (H - 1) * NHPD[0] + (P - 1) * NHPD[1] + D) * ES
    assert pool_bytes == NPAGES * PAGE * ES
    dspan = ((B - 1) * H * n * D + (H - 1) * n * D + (n - 1) * D + D) * ES
    assert _plan(_layer(False, k_out=POOL_K + pool_bytes), _pages(False), _dest()) == 0
    assert _plan(_layer(False, k_out=POOL_K + pool_bytes - 16), _pages(False), _dest()) == E_ARG
    assert _plan(_layer(False, k_out=POOL_K - dspan), _pages(False), _dest()) == 0
    assert _plan(_layer(False, k_out=POOL_K - dspan + 16), _pages(False), _dest()) == E_ARG
    assert _plan(_layer(False, v_out=POOL_K + 16), _pages(False), _dest()) == E_ARG
    assert _plan(_layer(False, k_out=POOL_V + pool_bytes - 16), _pages(False), _dest()) == E_ARG
    # fewer declared pages, shorter span
    assert _plan(_layer(False, k_out=POOL_K + pool_bytes - 16), _pages(False, num_pages=NPAGES - 1),
                 _dest()) == 0


@pytest.mark.parametrize("flag", [N.FLAG_GATHER_FIXED, N.FLAG_GATHER_SELECTED])
def test_gather_part_flags_are_refused(flag):
    ext = dict(external_index=1, phases=N.PHASE_GATHER)
    for inplace in (False, True):
        assert _plan(_layer(inplace), _pages(inplace), **ext) == 0
        assert _plan(_layer(inplace), _pages(inplace), flags=flag, **ext) == E_ARG
    assert _plan(_layer(False), _pages(False), flags=N.FLAG_SHARED_INDEX, **ext) == 0
