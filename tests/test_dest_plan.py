"""kvc_plan_dest's host-side contract (include/kvc.h, "Caller-provided destinations"): every
validation rule gives its stated code, and destinations never change what kvc_plan fills in.
CPU only: kvc_plan_dest is a pure host function (the pointers are never dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest

from kvcompress import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_ALIGN = -1, -4
B, H, D, ES = 2, 3, 64, 2
S, SMAX = 1000, 1037
SRC_K, SRC_V = 4 << 20, 8 << 20        # two static caches [B, H, SMAX, D] (under 1 MiB each)
DST_K, DST_V = 16 << 20, 24 << 20      # two more, far away
STATIC = (H * SMAX * D, SMAX * D, D)   # element strides of a window of a static cache
BSHD = (SMAX * H * D, D, H * D)        # the same rows stored [B, S, H, D]


def _params(**kw):
    d = dict(dtype=N.KVC_BF16, batch=B, heads=H, head_dim=D, order=0, algo=0, phases=N.PHASE_ALL,
             external_index=0)
    d.update(kw)
    return N.Params(**d)


def _layer(inplace, sink=4, zs=4, zl=700, k=100, ts=704, tl=296, **kw):
    t = np.zeros(1, dtype=N.LAYER_DTYPE)[0]
    t["k"], t["v"] = SRC_K, SRC_V
    t["k_out"], t["v_out"] = (SRC_K, SRC_V) if inplace else (DST_K, DST_V)
    t["k_stride"], t["v_stride"] = STATIC, BSHD
    t["seq_len"], t["zone_start"], t["zone_len"], t["n_select"] = S, zs, zl, k
    t["sink_len"], t["tail_start"], t["tail_len"] = sink, ts, tl
    for name, val in kw.items():
        t[name] = val
    return t


def _dest(inplace, ks=None, vs=None, **kw):
    d = np.zeros(1, dtype=N.DEST_DTYPE)[0]
    d["k_stride"] = ks if ks is not None else STATIC
    d["v_stride"] = vs if vs is not None else BSHD
    d["in_place"] = int(inplace)
    for name, val in kw.items():
        d[name] = val
    return d


def _plan(layer, dest, **pkw):
    table = np.array([layer], dtype=N.LAYER_DTYPE)
    dests = np.array([dest], dtype=N.DEST_DTYPE)
    rc, info = N.plan_dest(_params(**pkw), table, dests)
    return rc, info, table


def _info(i):
    return tuple(getattr(i, f) for f, _ in N.PlanInfo._fields_)


def test_struct_size_and_declarations():
    assert N.DEST_DTYPE.itemsize == 56
    hdr = open(os.path.join(ROOT, "include", "kvc.h")).read()
    flat = " ".join(hdr.split())
    assert re.search(r"int kvc_plan_dest\(const kvc_params_t\* params, kvc_layer_t\* layers, "
                     r"const kvc_dest_t\* dests, int num_layers, kvc_plan_info_t\* info\);", flat)
    assert re.search(r"int kvc_launch_dest\(const kvc_params_t\* params, const kvc_layer_t\* "
                     r"layers, const kvc_dest_t\* dests, int num_layers, void\* workspace, "
                     r"size_t workspace_bytes, kvc_stream_t stream\);", flat)
    assert "} kvc_dest_t;" in hdr
    text = " ".join(re.sub(r"\s*\n \*\s*", " ", hdr).split())
    assert "rows [n_out, S) and all bytes outside the written rows stay untouched" in text
    assert "is the caller's promise" in text
    assert {"kvc_plan_dest", "kvc_launch_dest"} <= set(N.EXPORTS)
    assert N.lib().kvc_version() == 4 and N.lib().kvc_layer_struct_size() == 136


def test_valid_tables_plan_like_kvc_plan():
    """dests = NULL, a valid in-place table and a valid strided table fill the same layer fields
    and the same kvc_plan_info_t as kvc_plan."""
    def table(inplace):
        return np.array([_layer(inplace), _layer(inplace, zl=600, k=600, ts=700, tl=300),
                         _layer(inplace, sink=4, zs=0, zl=0, k=0, ts=500, tl=500)],
                        dtype=N.LAYER_DTYPE)
    want = table(False)
    rc, winfo = N.plan(_params(), want)
    assert rc == 0
    t0 = table(False)
    rc, info = N.plan_dest(_params(), t0, None)
    assert rc == 0 and _info(info) == _info(winfo) and t0.tobytes() == want.tobytes()
    for inplace in (False, True):
        t = table(inplace)
        dests = np.array([_dest(inplace)] * 3, dtype=N.DEST_DTYPE)
        rc, info = N.plan_dest(_params(), t, dests)
        assert rc == 0, inplace
        assert _info(info) == _info(winfo)
        for f in ("n_out", "row0", "tile0", "unit0"):
            assert list(t[f]) == list(want[f]), (inplace, f)
    # launch re-validates the destinations before it touches the device (workspace NULL comes
    # after validation: a bad destination is reported first)
    t = table(True)
    dests = np.array([_dest(True)] * 3, dtype=N.DEST_DTYPE)
    assert N.plan_dest(_params(), t, dests)[0] == 0
    dests[1]["reserved"] = 1
    assert N.launch_dest(_params(), t, dests, None, 0, None) == E_ARG
    dests[1]["reserved"] = 0
    assert N.launch_dest(_params(), t, dests, None, 0, None) == -6  # KVC_E_WORKSPACE


@pytest.mark.parametrize("inplace", [False, True])
def test_reserved_and_in_place_values(inplace):
    assert _plan(_layer(inplace), _dest(inplace))[0] == 0
    assert _plan(_layer(inplace), _dest(inplace, reserved=1))[0] == E_ARG
    assert _plan(_layer(inplace), _dest(inplace, in_place=2))[0] == E_ARG
    assert _plan(_layer(inplace), _dest(inplace, in_place=-1))[0] == E_ARG


@pytest.mark.parametrize("side", ["ks", "vs"])
@pytest.mark.parametrize("dim", [0, 1, 2])
def test_destination_stride_alignment(dim, side):
    """A destination stride of a dim larger than 1 must be a multiple of 16 bytes; batch and
    heads of size 1, and the seq dim of a one-row output, are exempt."""
    base = {"ks": STATIC, "vs": BSHD}[side]
    bad = list(base)
    bad[dim] += 4  # 8 bytes off
    assert _plan(_layer(False), _dest(False, **{side: tuple(bad)}))[0] == E_ALIGN
    one = dict(batch=1) if dim == 0 else dict(heads=1) if dim == 1 else {}
    lay = _layer(False) if dim < 2 else _layer(False, sink=1, zs=1, zl=0, k=0, ts=0, tl=0)
    if dim == 2:
        assert lay["sink_len"] + lay["n_select"] + lay["tail_len"] == 1
    assert _plan(lay, _dest(False, **{side: tuple(bad)}), **one)[0] == 0


def test_in_place_must_name_the_input():
    ok = _layer(True)
    assert _plan(ok, _dest(True))[0] == 0
    assert _plan(_layer(True, k_out=DST_K), _dest(True))[0] == E_ARG
    assert _plan(_layer(True, v_out=DST_V), _dest(True))[0] == E_ARG
    other = (STATIC[0] + 8 * D, STATIC[1], STATIC[2])
    assert _plan(ok, _dest(True, ks=other))[0] == E_ARG
    assert _plan(ok, _dest(True, vs=(BSHD[0], BSHD[1] + 8, BSHD[2])))[0] == E_ARG


def test_in_place_needs_ordered_segments():
    """The row map must be strictly increasing with src(t) >= t."""
    cases = [
        (dict(sink=8, zs=4), E_ARG),                        # sink reaches into the zone
        (dict(sink=0, zs=0, zl=800, k=100, ts=700), E_ARG),  # zone reaches into the tail
        (dict(sink=4, zs=0, zl=0, k=0, ts=0, tl=1000), E_ARG),  # streaming_llm(recent_size=0)
        (dict(sink=8, zs=4, k=0), 0),                       # nothing selected: the zone is unused
        (dict(sink=4, zs=4, zl=700, k=100, ts=0, tl=0), 0),  # no tail: tail_start is unused
        (dict(sink=0, zs=0, zl=1000, k=900, ts=0, tl=0), 0),
    ]
    for kw, code in cases:
        assert _plan(_layer(True, **kw), _dest(True))[0] == code, kw
        assert _plan(_layer(False, **kw), _dest(False))[0] == 0, kw  # fine out of place


def test_in_place_refuses_zero_strides():
    for side in ("k", "v"):
        for dim in (0, 1, 2):
            st = list(STATIC if side == "k" else BSHD)
            st[dim] = 0
            lay = _layer(True, **{side + "_stride": tuple(st)})
            dst = _dest(True, **{side + "s": tuple(st)})
            assert _plan(lay, dst)[0] == E_ARG, (side, dim)
            assert N.plan(_params(), np.array([lay], dtype=N.LAYER_DTYPE))[0] == 0  # as an input
    st = (0,) + STATIC[1:]  # batch of one: its stride is never stepped over
    assert _plan(_layer(True, k_stride=st), _dest(True, ks=st), batch=1)[0] == 0


def test_destination_span_must_not_meet_the_sources():
    n_out = 400
    span_k = ((B - 1) * STATIC[0] + (H - 1) * STATIC[1] + (S - 1) * STATIC[2] + D) * ES
    span_v = ((B - 1) * BSHD[0] + (H - 1) * BSHD[1] + (S - 1) * BSHD[2] + D) * ES
    dspan_k = ((B - 1) * STATIC[0] + (H - 1) * STATIC[1] + (n_out - 1) * STATIC[2] + D) * ES
    assert _plan(_layer(False), _dest(False))[0] == 0
    assert _plan(_layer(False, k_out=SRC_K + span_k), _dest(False))[0] == 0  # just behind K
    assert _plan(_layer(False, k_out=SRC_K + span_k - 16), _dest(False))[0] == E_ARG
    assert _plan(_layer(False, k_out=SRC_K - dspan_k), _dest(False))[0] == 0  # just before K
    assert _plan(_layer(False, k_out=SRC_K - dspan_k + 16), _dest(False))[0] == E_ARG
    assert _plan(_layer(False, k_out=SRC_V + span_v - 16), _dest(False))[0] == E_ARG  # K dst, V src
    assert _plan(_layer(False, v_out=SRC_K + 16), _dest(False))[0] == E_ARG           # V dst, K src
    assert _plan(_layer(False, v_out=SRC_V), _dest(False))[0] == E_ARG
    # conservative: rows [S, SMAX) of the source's own cache lie inside the source's span
    assert _plan(_layer(False, k_out=SRC_K + S * D * ES), _dest(False))[0] == E_ARG
    # a layer without output is exempt
    empty = _layer(False, sink=0, zs=0, zl=0, k=0, ts=0, tl=0, k_out=SRC_K, v_out=SRC_V)
    assert _plan(empty, _dest(False, reserved=7))[0] == 0


@pytest.mark.parametrize("flag", [N.FLAG_GATHER_FIXED, N.FLAG_GATHER_SELECTED])
def test_gather_part_flags_are_refused_with_destinations(flag):
    lay = _layer(False)
    table = np.array([lay], dtype=N.LAYER_DTYPE)
    p = _params(external_index=1, phases=N.PHASE_GATHER, flags=flag)
    assert N.plan_dest(p, table.copy(), None)[0] == 0
    assert N.plan_dest(p, table.copy(), np.array([_dest(False)], dtype=N.DEST_DTYPE))[0] == E_ARG
