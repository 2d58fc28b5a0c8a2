"""kvc_plan_repage's host-side contract (include/kvc.h, "Paged destinations"): every validation
rule gives its stated code beside an accepting neighbour, pdests = NULL is kvc_plan_scaled, and a
destination table never changes what the in-place plan fills in.  CPU only: kvc_plan_repage is a
pure host function (no pointer is dereferenced).  And kvcompress.paged.check_repage_tables."""
import os

import numpy as np
import pytest

import test_abi
import test_paged_plan as PP
from kvcompress import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DTYPE, E_ALIGN = -1, -2, -4
B, H, D = PP.B, PP.H, PP.D
PD, NPD = 32, 40                           # destination page size / pool size
DTABLE = 2 << 20
SEQS, SEQS_DEV = 3 << 20, 3 << 20 | 1 << 12
SC_K, SC_V, DSC_K, DSC_V = 32 << 20, 33 << 20, 34 << 20, 35 << 20
N_OUT = 4 + 100 + 296


def _pdest(**kw):
    d = np.zeros(1, dtype=N.PAGE_DEST_DTYPE)[0]
    d["block_table"], d["table_stride"] = DTABLE, -(-N_OUT // PD)
    d["k_page_stride"] = d["v_page_stride"] = H * PD * D
    d["k_stride"], d["v_stride"] = (PD * D, D), (D, H * D)
    d["page_size"], d["num_pages"] = PD, NPD
    for name, val in kw.items():
        d[name] = val
    return d


def _scales(k=SC_K, v=SC_V, P=PP.P, flags=0, **kw):
    z = np.zeros(1, dtype=N.SCALES_DTYPE)[0]
    z["k_scale"], z["v_scale"] = k, v
    z["k_page_stride"] = z["v_page_stride"] = H * P
    z["k_stride"], z["v_stride"] = (P, 1), (1, H)
    z["flags"] = flags
    for name, val in kw.items():
        z[name] = val
    return z


def _plan(pdest, layer=None, pages=None, scales=None, dscales=None, ragged=None, info=False, **pkw):
    layer = PP._layer(False) if layer is None else layer
    pages = PP._pages(False) if pages is None else pages
    if scales is not None:
        pkw.setdefault("dtype", N.KVC_F8E4M3)
    arr = lambda x, dt: None if x is None else np.array([x], dtype=dt)  # noqa: E731
    table = np.array([layer], dtype=N.LAYER_DTYPE)
    rc, i = N.plan_repage(PP._params(**pkw), table, arr(pages, N.PAGES_DTYPE), ragged,
                          arr(scales, N.SCALES_DTYPE), arr(pdest, N.PAGE_DEST_DTYPE),
                          arr(dscales, N.SCALES_DTYPE))
    return (rc, i, table) if info else rc


def test_struct_size_and_declarations():
    assert N.PAGE_DEST_DTYPE.itemsize == 72
    assert {"kvc_plan_repage", "kvc_launch_repage"} <= set(N.EXPORTS)
    assert {"kvc_plan_repage", "kvc_launch_repage"} <= set(test_abi._declared_functions())
    hdr = open(os.path.join(ROOT, "include", "kvc.h")).read()
    assert "} kvc_page_dest_t;            /* 72 bytes */" in hdr
    assert hasattr(N.lib(), "kvc_plan_repage") and hasattr(N.lib(), "kvc_launch_repage")
    # the C struct's size, through the library: entry 1 of a two-layer table is read where numpy
    # put it (a bad field there is seen, a good one accepted)
    two = lambda x: np.array([x, x], dtype=N.PAGE_DEST_DTYPE)  # noqa: E731
    table = np.array([PP._layer(False)] * 2, dtype=N.LAYER_DTYPE)
    pages = np.array([PP._pages(False)] * 2, dtype=N.PAGES_DTYPE)
    pd = two(_pdest())
    assert N.plan_repage(PP._params(), table, pages, None, None, pd, None)[0] == 0
    pd[1]["num_pages"] = 0
    assert N.plan_repage(PP._params(), table, pages, None, None, pd, None)[0] == E_ARG


def test_accepts_and_fills_the_in_place_plan():
    rc, info, table = _plan(_pdest(), info=True)
    assert rc == 0
    t0 = np.array([PP._layer(True)], dtype=N.LAYER_DTYPE)
    rc0, info0 = N.plan_paged(PP._params(), t0, np.array([PP._pages(True)], dtype=N.PAGES_DTYPE))
    assert rc0 == 0 and PP._info(info) == PP._info(info0)
    for f in ("n_out", "row0", "tile0", "unit0"):
        assert table[0][f] == t0[0][f]
    assert table[0]["n_out"] == N_OUT
    # the destination pool may be the source pool; a wider table_stride is fine
    assert _plan(_pdest(table_stride=99), layer=PP._layer(True)) == 0


def test_pdests_null_is_kvc_plan_scaled():
    for inplace, scales in ((True, None), (False, None), (True, _scales())):
        pkw = dict(dtype=N.KVC_F8E4M3) if scales is not None else {}
        arr = None if scales is None else np.array([scales], dtype=N.SCALES_DTYPE)
        t0 = np.array([PP._layer(inplace)], dtype=N.LAYER_DTYPE)
        t1 = t0.copy()
        pages = np.array([PP._pages(inplace)], dtype=N.PAGES_DTYPE)
        rc0, i0 = N.plan_scaled(PP._params(**pkw), t0, pages, None, arr)
        rc1, i1 = N.plan_repage(PP._params(**pkw), t1, pages, None, arr, None, None)
        assert rc0 == rc1 == 0 and PP._info(i0) == PP._info(i1) and t0.tobytes() == t1.tobytes()
    # ... errors included: an in-place scaled layer with a dense output
    t = np.array([PP._layer(False)], dtype=N.LAYER_DTYPE)
    pages = np.array([PP._pages(False)], dtype=N.PAGES_DTYPE)
    z = np.array([_scales()], dtype=N.SCALES_DTYPE)
    p = PP._params(dtype=N.KVC_F8E4M3)
    assert N.plan_scaled(p, t, pages, None, z)[0] == \
        N.plan_repage(p, t, pages, None, z, None, None)[0] == E_ARG


BAD = [  # (field changes that break one rule, code); _pdest() itself is the accepting neighbour
    (dict(block_table=0), E_ARG), (dict(block_table=DTABLE + 2), E_ARG),
    (dict(page_size=0), E_ARG), (dict(page_size=24), E_ARG), (dict(page_size=131072), E_ARG),
    (dict(num_pages=0), E_ARG), (dict(table_stride=-(-N_OUT // PD) - 1), E_ARG),
    (dict(k_stride=(0, D)), E_ARG), (dict(v_stride=(D, 0)), E_ARG), (dict(k_page_stride=0), E_ARG),
    (dict(k_stride=(PD * D + 4, D)), E_ALIGN), (dict(v_stride=(D, H * D + 4)), E_ALIGN),
    (dict(v_page_stride=H * PD * D + 4), E_ALIGN),
]


@pytest.mark.parametrize("change, code", BAD, ids=[str(c) for c, _ in BAD])
def test_destination_rules(change, code):
    assert _plan(_pdest()) == 0
    assert _plan(_pdest(**change)) == code


def test_neighbours_that_are_accepted():
    """The rules bind dims larger than 1 only, and the page-size bounds are inclusive."""
    assert _plan(_pdest(page_size=65536, table_stride=1)) == 0
    assert _plan(_pdest(page_size=1, table_stride=N_OUT, k_stride=(D, 0), v_stride=(D, 4))) == 0
    assert _plan(_pdest(num_pages=1, k_page_stride=0, v_page_stride=4)) == 0
    assert _plan(_pdest(k_stride=(0, D), v_stride=(4, H * D)), heads=1,
                 layer=PP._layer(False, k_stride=(0, 0, D), v_stride=(0, 0, D))) == 0
    # a layer without output is exempt
    empty = PP._layer(False, sink_len=0, n_select=0, tail_len=0)
    assert _plan(_pdest(block_table=0, page_size=3), layer=empty) == 0


def test_layer_rules():
    assert _plan(_pdest(), pages=PP._pages(True), layer=PP._layer(True)) == E_ARG  # in_place == 1
    assert _plan(_pdest(), layer=PP._layer(False, k_out=PP.DST_K + 8)) == E_ALIGN
    assert _plan(_pdest(), layer=PP._layer(False, v_out=0)) == E_ARG
    assert _plan(_pdest(), flags=N.FLAG_GATHER_FIXED, external_index=1) == E_ARG
    assert _plan(_pdest(), external_index=1) == 0
    assert _plan(_pdest(), external_index=1, flags=N.FLAG_SHARED_INDEX) == 0
    # no segment-order rule out of place: a zone before the sink (refused in place) is accepted
    odd = dict(sink=8, zs=0, zl=700, k=100, ts=704, tl=296)
    assert _plan(_pdest(table_stride=13), layer=PP._layer(False, **odd)) == 0
    assert PP._plan(PP._layer(True, **odd), PP._pages(True)) == E_ARG


def test_scale_rules():
    z = _scales()
    dz = _scales(DSC_K, DSC_V, PD)
    assert _plan(_pdest(), scales=z, dscales=dz) == 0
    assert _plan(_pdest(), scales=z, dscales=dz, dtype=N.KVC_BF16) == E_DTYPE
    assert _plan(_pdest(), scales=z, dscales=None) == E_ARG
    assert _plan(_pdest(), scales=z, dscales=_scales(0, DSC_V, PD)) == E_ARG
    assert _plan(_pdest(), scales=z, dscales=_scales(DSC_K + 2, DSC_V, PD)) == E_ALIGN
    assert _plan(_pdest(), scales=z, dscales=_scales(DSC_K, DSC_V, PD, k_stride=(0, 1))) == E_ARG
    assert _plan(_pdest(), scales=z, dscales=_scales(DSC_K, DSC_V, PD, v_stride=(1, 0))) == E_ARG
    assert _plan(_pdest(), scales=z, dscales=_scales(DSC_K, DSC_V, PD, v_page_stride=0)) == E_ARG
    assert _plan(_pdest(), scales=z, dscales=_scales(DSC_K, DSC_V, PD, reserved=1)) == E_ARG
    # the flags of a side must match; a uniform / absent side's destination pointer is not read
    uni = N.SCALE_K_UNIFORM | N.SCALE_V_NONE
    assert _plan(_pdest(), scales=_scales(flags=uni), dscales=dz) == E_ARG
    assert _plan(_pdest(), scales=_scales(flags=uni),
                 dscales=_scales(0, 0, PD, flags=uni, k_stride=(0, 0), v_stride=(0, 0))) == 0
    assert _plan(_pdest(), scales=z, dscales=_scales(DSC_K, DSC_V, PD, flags=uni)) == E_ARG


def _ragged(recs):
    host = np.zeros(len(recs), dtype=N.SEQ_DTYPE)
    for i, r in enumerate(recs):
        host[i] = r
    rg = np.zeros(1, dtype=N.RAGGED_DTYPE)
    rg[0] = (host.ctypes.data, SEQS_DEV)
    return host, rg


def test_ragged_rules():
    # (seq_len, zone_start, zone_len, n_select, sink, tail_start, tail_len, mode, pool, n_out, res)
    good = (1000, 4, 700, 100, 4, 704, 296, 0, 0, 400, (0, 0))
    other = (600, 0, 0, 0, 0, 0, 0, 0, 0, 0, (0, 0))        # n_out == 0: another group's sequence
    host, rg = _ragged([good, other])
    assert _plan(_pdest(), ragged=rg) == 0
    assert _plan(_pdest(table_stride=12), ragged=rg) == E_ARG    # the LARGEST n_out decides
    assert _plan(_pdest(), ragged=rg, pages=PP._pages(True), layer=PP._layer(True)) == E_ARG
    assert _plan(_pdest(), ragged=rg, external_index=1) == E_ARG
    unordered = (1000, 0, 700, 100, 8, 704, 296, 0, 0, 404, (0, 0))  # refused in place
    host2, rg2 = _ragged([unordered, other])
    assert _plan(_pdest(), ragged=rg2) == 0
    t = np.array([PP._layer(True)], dtype=N.LAYER_DTYPE)
    assert N.plan_ragged(PP._params(), t, np.array([PP._pages(True)], dtype=N.PAGES_DTYPE),
                         rg2)[0] == E_ARG
    # plan info equals the in-place ragged plan's for the same records
    passing = (600, 0, 0, 0, 600, 0, 0, 0, 0, 600, (0, 0))
    host3, rg3 = _ragged([good, passing])
    rc, info, _ = _plan(_pdest(table_stride=19), ragged=rg3, info=True)
    t = np.array([PP._layer(True)], dtype=N.LAYER_DTYPE)
    rc0, info0 = N.plan_ragged(PP._params(), t, np.array([PP._pages(True)], dtype=N.PAGES_DTYPE),
                               rg3)
    assert rc == rc0 == 0 and PP._info(info) == PP._info(info0)
    assert len(host) == len(host2) == len(host3) == 2


def test_launch_revalidates_and_stops_at_the_workspace():
    table = np.array([PP._layer(False)], dtype=N.LAYER_DTYPE)
    pages = np.array([PP._pages(False)], dtype=N.PAGES_DTYPE)
    pd = np.array([_pdest()], dtype=N.PAGE_DEST_DTYPE)
    p = PP._params()
    assert N.plan_repage(p, table, pages, None, None, pd, None)[0] == 0
    assert N.launch_repage(p, table, pages, None, None, pd, None, None, 0, None) == -6
    pd[0]["page_size"] = 3
    assert N.launch_repage(p, table, pages, None, None, pd, None, None, 0, None) == E_ARG


# ---- check_repage_tables ---------------------------------------------------------------------
def test_check_repage_tables():
    from kvcompress.paged import check_repage_tables
    src = np.array([[0, 1, 2, 3], [0, 1, 4, 5]])        # a shared prefix of two pages
    dst = np.array([[6, 7, -1], [8, 9, -1]])
    check_repage_tables(src, [60, 64], 16, dst, 32, 16)
    check_repage_tables(src, [60, 64], 16, dst, [17, 32], 16)
    with pytest.raises(ValueError, match="page 3 is destination page 1 of sequence 0 and a source "
                                         "page of sequence 0"):
        check_repage_tables(src, [60, 64], 16, np.array([[6, 3, -1], [8, 9, -1]]), 32, 16)
    with pytest.raises(ValueError, match="page 6 is a destination page twice: of sequence 0 and "
                                         "of sequence 1"):
        check_repage_tables(src, [60, 64], 16, np.array([[6, 7, -1], [8, 6, -1]]), 32, 16)
    # entries past the lengths are ignored: source page 3 is beyond 48 rows, destination column 1
    # beyond 16
    check_repage_tables(src, [48, 64], 16, np.array([[6, 3, -1], [8, 9, -1]]), [32, 32], 16)
    check_repage_tables(src, [60, 64], 16, np.array([[6, 3, -1], [8, 6, -1]]), 16, 16)
    with pytest.raises(ValueError, match="source page"):  # the in-place tables of the same call
        check_repage_tables(src, [60, 64], 16, src, 32, 16)
