"""Compression into caller-provided destinations on the GPU (include/kvc.h, "Caller-provided
destinations"; the `out` kwarg of every compress function): compaction in place at the front of
a static cache, strided destinations, the two C entries, and the errors that need device tensors.

Expected bytes come from the CPU oracle on the contiguous numpy inputs (tests/dest_cases.py; the
row maps of the in-place cases are proved hazardous for an unordered copy, and safe for the
kernel's schedule, in tests/test_dest_order.py).  Every input is a window [:, :, :S] of a
poison-filled cache of S + 37 rows -- K stored [B, H, S_max, D], V stored [B, S_max, H, D], so
their stride triples differ -- and every check compares the WHOLE backing buffers against a copy
taken before the call with the oracle's rows written into it: the returned bytes, and every byte
the call must not touch, in one comparison.
"""
import copy

import numpy as np
import pytest
import torch

import dest_cases as DC
import phase_tables as PT
import prng
import strided_layouts as SL
from gpu_util import to_dev, to_np
from kvcompress import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT = {2: torch.int16, 4: torch.int32}


def _method(name):
    from kvcompress.methods import get_compress_fn
    if name == "evict_for_space":
        from kvcompress.methods.streaming_llm import evict_for_space
        return evict_for_space
    return get_compress_fn(name)


def _ints(t):
    return t.view(INT[t.element_size()])


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _window(backing, layout, S, start=0):
    """The [B, H, S, D] window at row `start` of a cache stored in `layout`."""
    v = backing if layout == "static" else backing.permute(0, 2, 1, 3)
    return v[:, :, start:start + S]


def _cache(shape, dtype, layout, pad=SL.STATIC_PAD):
    """An all-poison cache of S + pad rows for [B, H, S, D] windows."""
    B, H, S, D = shape
    if layout == "static":
        return SL.new_backing("static", (B, H, S + pad - SL.STATIC_PAD, D), dtype, DEV)
    return SL.new_backing("bshd", (B, H, S + pad, D), dtype, DEV)


def _filled(a_np, layout):
    """(cache, window [:, :, :S] holding a_np)."""
    src = to_dev(a_np, DEV)
    back = _cache(tuple(src.shape), src.dtype, layout)
    win = _window(back, layout, src.shape[2])
    win.copy_(src)
    assert win.data_ptr() == back.data_ptr() and not win.is_contiguous()
    return back, win


def _policy(monkeypatch, case):
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "tie_policy", case["tie"])


def _check_inplace(case, fill=0):
    layers, ref = DC.reference(case, tagged=True, fill=fill)
    caches = [(_filled(k, "static"), _filled(v, "bshd")) for k, v in layers]
    tin = [(kc[1], vc[1]) for kc, vc in caches]
    before = [(kc[0].clone(), vc[0].clone()) for kc, vc in caches]
    assert all(k.stride()[:3] != v.stride()[:3] for k, v in tin)
    out = _method(case["method"])(list(tin), out="inplace", **case["kw"])
    torch.cuda.synchronize()
    assert len(out) == len(ref)
    for li, ((ki, vi), (ko, vo), (rk, rv, kind)) in enumerate(zip(tin, out, ref)):
        ctx = (case["id"], fill, li)
        if kind == "same":
            assert out[li] is tin[li] or (ko is ki and vo is vi), ctx
            n = 0
        else:
            n = rk.shape[2]
            for x, y in ((ki, ko), (vi, vo)):
                assert y.data_ptr() == x.data_ptr() and y.stride() == x.stride(), ctx
                assert tuple(y.shape) == tuple(x.shape[:2]) + (n, x.shape[3]), ctx
            assert np.array_equal(_bytes(to_np(ko)), _bytes(rk)), ctx + ("K",)
            assert np.array_equal(_bytes(to_np(vo)), _bytes(rv)), ctx + ("V",)
        for back, was, want, layout in ((caches[li][0][0], before[li][0], rk, "static"),
                                        (caches[li][1][0], before[li][1], rv, "bshd")):
            if n:
                _window(was, layout, n).copy_(to_dev(want, DEV))
            assert torch.equal(_ints(back), _ints(was)), ctx + (layout, "bytes outside rows [0, n)")
    return out


@pytest.mark.parametrize("case", DC.INPLACE, ids=[c["id"] for c in DC.INPLACE])
def test_compaction_in_place(case, monkeypatch):
    """Cases 1-8, 10-12 and 14 of the issue; those with repeat = 3 run three times on freshly
    filled buffers of the same shapes."""
    _policy(monkeypatch, case)
    kinds = set()
    for fill in range(case["repeat"]):
        _check_inplace(case, fill)
        kinds |= {kind for _, _, kind in DC.reference(case, True, fill)[1]}
    want = {"recent_only-512": {"view"}, "snapkv_lite-window-only": {"view"},
            "fix_size_l2-skip0-and-short": {"same", "new"}}.get(case["id"], {"new"})
    assert kinds == want, case["id"]


def test_random_strategy_in_place():
    """Case 9: caller-side indices (strategy="random", the external index region).  Expected: the
    default call on cloned inputs under the same torch seed."""
    from kvcompress.methods import fix_size_l2_compress
    shape = (DC.B, DC.H, 1500, 64)
    kn, vn = prng.gen_keys(41090, shape, "bf16"), prng.encode_positions(shape, "bf16")
    (kb, k), (vb, v) = _filled(kn, "static"), _filled(vn, "bshd")
    kw = dict(fix_kv_size=512, keep_ratio=0.25, strategy="random", skip_layers=[])
    torch.manual_seed(77)
    want = fix_size_l2_compress([(k.clone(), v.clone())], **kw)
    was = (kb.clone(), vb.clone())
    torch.manual_seed(77)
    out = fix_size_l2_compress([(k, v)], out="inplace", **kw)
    torch.cuda.synchronize()
    n = want[0][0].shape[2]
    assert n == 512
    for x, y, w, back, old, layout in ((k, out[0][0], want[0][0], kb, was[0], "static"),
                                       (v, out[0][1], want[0][1], vb, was[1], "bshd")):
        assert y.data_ptr() == x.data_ptr() and y.stride() == x.stride() and y.shape == w.shape
        _window(old, layout, n).copy_(w)
        assert torch.equal(_ints(back), _ints(old)), layout
    pos, ok = prng.decode_positions(to_np(out[0][1]), "bf16")
    assert ok and (np.diff(pos, axis=2) > 0).all() and not (pos[0, 0] == pos[1, 2]).all()


def _tie_attention(rng, shape, levels=4):
    logits = rng.integers(0, levels, size=shape).astype(np.float32) * np.float32(0.7)
    return torch.from_numpy(logits).softmax(dim=-1)


@pytest.mark.parametrize("mode", ["inplace", "strided"])
def test_h2o_attention_with_a_manager(mode):
    """Case 13: the shared index (one list per layer serves every head).  Expected: the default
    call on cloned inputs with a deep-copied manager.  B = 1 here: only then do the heavy hitters
    go from kvc_heavy_hitters straight into the index region (h2o_attention_compress takes that
    path for batch-1 accumulations); test_h2o_attention_host_indices covers B = 2."""
    from kvcompress.methods import h2o_attention as HA
    rng = np.random.default_rng(13)
    Hh, S, D, start, hh, recent = 3, 700, 64, 4, 64, 128
    kw = dict(start_size=start, heavy_hitter_size=hh, recent_size=recent)
    assert S - start - recent < HA.OVERLAP_MIN_ZONE
    layers = [(prng.gen_keys(41200 + i, (1, Hh, S, D), "bf16"),
               prng.gen_values(41200 + i, (1, Hh, S, D), "bf16")) for i in range(2)]
    caches = [(_filled(k, "static"), _filled(v, "bshd")) for k, v in layers]
    tin = [(kc[1], vc[1]) for kc, vc in caches]
    att = tuple(_tie_attention(rng, (1, Hh, 2, S)).to(torch.bfloat16).to(DEV) for _ in tin)
    mgr = HA.H2OAttentionManager(**kw)
    mgr2 = copy.deepcopy(mgr)
    want = HA.h2o_attention_compress([(k.clone(), v.clone()) for k, v in tin],
                                     attention_scores=att, h2o_manager=mgr2, **kw)
    n = start + hh + recent
    assert all(wk.shape == (1, Hh, n, D) for wk, _ in want)
    before = [(kc[0].clone(), vc[0].clone()) for kc, vc in caches]
    if mode == "inplace":
        dst, arg = caches, "inplace"
    else:
        dst = [(_dest((1, Hh, n + 5, D), torch.bfloat16, "static"),
                _dest((1, Hh, n + 5, D), torch.bfloat16, "bshd")) for _ in tin]
        arg = [(kd[1], vd[1]) for kd, vd in dst]
    dwas = [(kd[0].clone(), vd[0].clone()) for kd, vd in dst]
    out = HA.h2o_attention_compress(list(tin), attention_scores=att, h2o_manager=mgr, out=arg,
                                    **kw)
    torch.cuda.synchronize()
    for li in range(len(tin)):
        for j, layout in ((0, "static"), (1, "bshd")):
            ctx = (mode, li, layout)
            y, w = out[li][j], want[li][j]
            assert y.data_ptr() == dst[li][j][1].data_ptr() and y.shape == w.shape, ctx
            assert y.stride() == dst[li][j][1].stride(), ctx
            assert torch.equal(_ints(y.contiguous()), _ints(w.contiguous())), ctx
            y_rows = dst[li][j][1][:, :, :n]
            exp = dwas[li][j]
            exp_win = exp.as_strided(y_rows.shape, y_rows.stride(),
                                     y_rows.storage_offset() - dst[li][j][0].storage_offset())
            exp_win.copy_(w)
            assert torch.equal(_ints(dst[li][j][0]), _ints(exp)), ctx + ("bytes around",)
            if mode == "strided":
                assert torch.equal(_ints(caches[li][j][0]), _ints(before[li][j])), ctx + ("input",)
        assert torch.equal(mgr.accumulated_attention[li], mgr2.accumulated_attention[li])


# ---- strided destinations ---------------------------------------------------------------------
DST_START = {"static": SL.STATIC_START, "bshd": 7}


def _dest(shape, dtype, layout):
    """(poisoned backing, [B, H, S_d, D] window inside it): the window starts a few rows into a
    cache that is 37 rows longer, so poison lies on both sides of it."""
    back = _cache(shape, dtype, layout)
    win = _window(back, layout, shape[2], DST_START[layout])
    assert tuple(win.shape) == tuple(shape) and not win.is_contiguous()
    return back, win


@pytest.mark.parametrize("case", DC.STRIDED, ids=[c["id"] for c in DC.STRIDED])
def test_strided_destinations(case, monkeypatch):
    """Cases 3, 4, 7, 11 and 14 into a second cache: the K destination stored [B, H, S, D], the V
    destination [B, S, H, D], S_d = n_out + 5.  Layers the method leaves alone or slices are
    copied; the poison around the written rows and the inputs stay as they were."""
    _policy(monkeypatch, case)
    layers, ref = DC.reference(case, tagged=False)
    caches = [(_filled(k, "static"), _filled(v, "bshd")) for k, v in layers]
    tin = [(kc[1], vc[1]) for kc, vc in caches]
    before = [(kc[0].clone(), vc[0].clone()) for kc, vc in caches]
    dst = []
    for (k, v), (rk, rv, kind) in zip(tin, ref):
        shape = tuple(k.shape[:2]) + (rk.shape[2] + 5, k.shape[3])
        dst.append((_dest(shape, k.dtype, "static"), _dest(shape, k.dtype, "bshd")))
    dwas = [(kd[0].clone(), vd[0].clone()) for kd, vd in dst]
    out = _method(case["method"])(list(tin), out=[(kd[1], vd[1]) for kd, vd in dst],
                                  **case["kw"])
    torch.cuda.synchronize()
    for li, ((ko, vo), (rk, rv, kind)) in enumerate(zip(out, ref)):
        n = rk.shape[2]
        for j, (y, want, layout) in enumerate(((ko, rk, "static"), (vo, rv, "bshd"))):
            ctx = (case["id"], li, kind, layout)
            back, win = dst[li][j]
            assert y.data_ptr() == win.data_ptr() and y.stride() == win.stride(), ctx
            assert tuple(y.shape) == want.shape, ctx
            assert np.array_equal(_bytes(to_np(y)), _bytes(want)), ctx
            exp = dwas[li][j]
            _window(exp, layout, n, DST_START[layout]).copy_(to_dev(want, DEV))
            assert torch.equal(_ints(back), _ints(exp)), ctx + ("poison around the rows",)
            assert torch.equal(_ints(caches[li][j][0]), _ints(before[li][j])), ctx + ("input",)
    if case["id"] == "fix_size_l2-skip0-and-short":
        assert [kind for _, _, kind in ref] == ["same", "new", "same", "new"]


def test_sliced_results_are_copied_into_their_destination():
    """recent_only returns views of its input by default; with a destination they are copied."""
    from kvcompress.methods import recent_only_compress
    shape = (DC.B, DC.H, 700, 64)
    kn, vn = prng.gen_keys(41300, shape, "bf16"), prng.gen_values(41300, shape, "bf16")
    (kb, k), (vb, v) = _filled(kn, "static"), _filled(vn, "bshd")
    (kdb, kd), (vdb, vd) = (_dest((DC.B, DC.H, 105, 64), k.dtype, lay) for lay in ("static", "bshd"))
    was = (kdb.clone(), vdb.clone())
    out = recent_only_compress([(k, v)], window_size=100, skip_layers=[], out=[(kd, vd)])
    torch.cuda.synchronize()
    for y, x, win, back, old, layout in ((out[0][0], kn, kd, kdb, was[0], "static"),
                                         (out[0][1], vn, vd, vdb, was[1], "bshd")):
        assert y.data_ptr() == win.data_ptr() and y.shape[2] == 100
        _window(old, layout, 100, DST_START[layout]).copy_(to_dev(x[:, :, -100:], DEV))
        assert torch.equal(_ints(back), _ints(old)), layout


# ---- the C entries ----------------------------------------------------------------------------
D_ABI = 64


def _abi_table(specs, dev, B, H, outs):
    table = np.zeros(len(specs), dtype=N.LAYER_DTYPE)
    for t, s, (k, v), (ko, vo) in zip(table, specs, dev, outs):
        t["k"], t["v"], t["k_out"], t["v_out"] = (x.data_ptr() for x in (k, v, ko, vo))
        t["k_stride"], t["v_stride"] = k.stride()[:3], v.stride()[:3]
        t["seq_len"], t["zone_start"], t["zone_len"] = s["S"], s["zone_start"], s["zone_len"]
        t["n_select"], t["sink_len"] = s["n_select"], s["sink"]
        t["tail_start"], t["tail_len"] = s["tail_start"], s["tail_len"]
        t["score_mode"], t["pool_kernel"] = s["score_mode"], s["pool"]
    return table


def _abi_call(B, H, flags=0):
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = N.Params(dtype=N.KVC_BF16, batch=B, heads=H, head_dim=D_ABI, order=PT.ASC, algo=PT.SORT,
                 phases=N.PHASE_ALL, external_index=0, flags=flags,
                 device_status=status.data_ptr())
    return p, status


def _workspace(info):
    return torch.full((int(info.workspace_bytes),), PT.POISON, dtype=torch.uint8, device=DEV)


def test_c_abi_launch_dest():
    """One four-layer table (a selecting layer, a copy-only one, a select-all one, a few-row
    selection) through _native: kvc_launch_dest with dests = NULL equals kvc_launch; the in-place
    table launched as three separate phases equals one KVC_PHASE_ALL launch on a second copy of
    the caches, equals the oracle, and leaves rows [n_out, S) alone."""
    Z = 1000
    B, H = PT.split_geometry(Z)
    specs = PT.split_table(Z)
    host = PT.gen_layers(specs, B, H, D_ABI, "bf16")
    want = [PT.expected_layer(k, v, s, PT.ASC, PT.SORT) for (k, v), s in zip(host, specs)]
    stream = torch.cuda.current_stream().cuda_stream

    # dests = NULL
    dev = [(to_dev(k, DEV), to_dev(v, DEV)) for k, v in host]
    got = []
    for entry in ("launch", "launch_dest"):
        outs = [tuple(torch.zeros((B, H, PT.n_out(s), D_ABI), dtype=torch.bfloat16, device=DEV)
                      for _ in range(2)) for s in specs]
        table = _abi_table(specs, dev, B, H, outs)
        p, status = _abi_call(B, H)
        rc, info = N.plan_dest(p, table, None)
        assert rc == 0
        ws = _workspace(info)
        if entry == "launch":
            rc = N.launch(p, table, ws.data_ptr(), int(info.workspace_bytes), stream)
        else:
            rc = N.launch_dest(p, table, None, ws.data_ptr(), int(info.workspace_bytes), stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        got.append(outs)
    for li, ((k0, v0), (k1, v1), (wk, wv, _)) in enumerate(zip(got[0], got[1], want)):
        assert torch.equal(_ints(k0), _ints(k1)) and torch.equal(_ints(v0), _ints(v1)), li
        assert np.array_equal(_bytes(to_np(k1)), _bytes(wk)), li

    # in place: three phases | one launch
    results = []
    for phase_list in ((N.PHASE_SCORE, N.PHASE_SELECT, N.PHASE_GATHER), (N.PHASE_ALL,)):
        dev = [(to_dev(k, DEV), to_dev(v, DEV)) for k, v in host]
        table = _abi_table(specs, dev, B, H, dev)
        dests = np.zeros(len(specs), dtype=N.DEST_DTYPE)
        dests["k_stride"], dests["v_stride"] = table["k_stride"], table["v_stride"]
        dests["in_place"] = 1
        p, status = _abi_call(B, H)
        rc, info = N.plan_dest(p, table, dests)
        assert rc == 0
        ws = _workspace(info)
        for ph in phase_list:
            p.phases = ph
            rc = N.launch_dest(p, table, dests, ws.data_ptr(), int(info.workspace_bytes), stream)
            assert rc == 0, ph
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        results.append(dev)
    for li, ((k0, v0), (k1, v1), (hk, hv), (wk, wv, _), s) in enumerate(
            zip(results[0], results[1], host, want, specs)):
        n = PT.n_out(s)
        assert torch.equal(_ints(k0), _ints(k1)) and torch.equal(_ints(v0), _ints(v1)), li
        for got_t, w, h in ((k1, wk, hk), (v1, wv, hv)):
            g = to_np(got_t)
            assert np.array_equal(_bytes(g[:, :, :n]), _bytes(w)), li
            assert np.array_equal(_bytes(g[:, :, n:]), _bytes(h[:, :, n:])), li


# ---- errors that need device tensors ----------------------------------------------------------
def test_errors_leave_the_inputs_untouched():
    from kvcompress.methods import fix_size_l2_compress, streaming_llm_compress
    shape = (DC.B, DC.H, 600, 64)
    kn, vn = prng.gen_keys(41400, shape, "bf16"), prng.gen_values(41400, shape, "bf16")
    (kb, k), (vb, v) = _filled(kn, "static"), _filled(vn, "bshd")
    was = (kb.clone(), vb.clone())
    kw = dict(fix_kv_size=100, keep_ratio=0.25, skip_layers=[])
    good = tuple(torch.zeros(DC.B, DC.H, 100, 64, dtype=torch.bfloat16, device=DEV)
                 for _ in range(2))
    with pytest.raises(ValueError, match="layer 0: V destination is on cpu"):
        fix_size_l2_compress([(k, v)], out=[(good[0], good[1].cpu())], **kw)
    with pytest.raises(ValueError, match="layer 0: K destination holds 99 rows"):
        fix_size_l2_compress([(k, v)], out=[(good[0][:, :, :99], good[1])], **kw)
    with pytest.raises(ValueError, match="layer 0: K destination overlaps the layer's K"):
        fix_size_l2_compress([(k, v)], out=[(_window(kb, "static", 100, 500), good[1])], **kw)
    with pytest.raises(ValueError, match="layer 0: V destination overlaps the layer's V"):
        fix_size_l2_compress([(k, v)], out=[(good[0], _window(vb, "bshd", 100, 500))], **kw)
    with pytest.raises(TypeError, match="layer 0: K destination has dtype"):
        fix_size_l2_compress([(k, v)], out=[(good[0].half(), good[1])], **kw)
    with pytest.raises(ValueError, match="layer 0: K.*stride 0"):
        fix_size_l2_compress([(k[:1].expand(*shape), v)], out="inplace", **kw)
    with pytest.raises(ValueError, match="layer 0: cannot be compacted in place"):
        streaming_llm_compress([(k, v)], start_size=4, recent_size=0, out="inplace")
    # a second layer's bad destination stops the call before the first layer is written
    with pytest.raises(ValueError, match="layer 1: K destination holds 99 rows"):
        fix_size_l2_compress([(k, v), (k.clone(), v.clone())],
                             out=["inplace", (good[0][:, :, :99], good[1])], **kw)
    torch.cuda.synchronize()
    assert torch.equal(_ints(kb), _ints(was[0])) and torch.equal(_ints(vb), _ints(was[1]))
    assert not good[0].any() and not good[1].any()


@pytest.mark.parametrize("mode", ["inplace", "strided"])
def test_h2o_attention_host_indices(mode):
    """B = 2, a manager that has seen no attention: every layer's shared index list comes from
    the host (evenly spaced middle positions) and is copied into the index region."""
    from kvcompress.methods import h2o_attention as HA
    S, D, start, hh, recent = 700, 64, 4, 64, 128
    kw = dict(start_size=start, heavy_hitter_size=hh, recent_size=recent)
    layers = [(prng.gen_keys(41250 + i, (DC.B, DC.H, S, D), "bf16"),
               prng.gen_values(41250 + i, (DC.B, DC.H, S, D), "bf16")) for i in range(2)]
    caches = [(_filled(k, "static"), _filled(v, "bshd")) for k, v in layers]
    tin = [(kc[1], vc[1]) for kc, vc in caches]
    want = HA.h2o_attention_compress([(k.clone(), v.clone()) for k, v in tin],
                                     h2o_manager=HA.H2OAttentionManager(**kw), **kw)
    n = start + hh + recent
    assert all(wk.shape == (DC.B, DC.H, n, D) for wk, _ in want)
    if mode == "inplace":
        dst, arg = caches, "inplace"
    else:
        dst = [(_dest((DC.B, DC.H, n + 5, D), torch.bfloat16, "static"),
                _dest((DC.B, DC.H, n + 5, D), torch.bfloat16, "bshd")) for _ in tin]
        arg = [(kd[1], vd[1]) for kd, vd in dst]
    dwas = [(kd[0].clone(), vd[0].clone()) for kd, vd in dst]
    out = HA.h2o_attention_compress(list(tin), h2o_manager=HA.H2OAttentionManager(**kw), out=arg,
                                    **kw)
    torch.cuda.synchronize()
    for li in range(len(tin)):
        for j, layout in ((0, "static"), (1, "bshd")):
            y, w, (back, win) = out[li][j], want[li][j], dst[li][j]
            assert y.data_ptr() == win.data_ptr() and y.stride() == win.stride(), (mode, li, layout)
            rows = win[:, :, :n]
            exp = dwas[li][j]
            exp.as_strided(rows.shape, rows.stride(),
                           rows.storage_offset() - back.storage_offset()).copy_(w)
            assert torch.equal(_ints(back), _ints(exp)), (mode, li, layout)


def test_a_failed_check_leaves_caches_and_manager_alone():
    """Every destination of a call -- of the layers the method compresses AND of those it passes
    through, whose copy comes last -- is checked before anything launches, and a manager that
    h2o_attention_compress has already updated gets its state back."""
    from kvcompress.methods import fix_size_l2_compress
    from kvcompress.methods import h2o_attention as HA
    shape = (DC.B, DC.H, 600, 64)
    layers = [(prng.gen_keys(41500 + i, shape, "bf16"), prng.gen_values(41500 + i, shape, "bf16"))
              for i in range(2)]
    caches = [(_filled(k, "static"), _filled(v, "bshd")) for k, v in layers]
    tin = [(kc[1], vc[1]) for kc, vc in caches]
    was = [(kc[0].clone(), vc[0].clone()) for kc, vc in caches]
    spare = [_dest((DC.B, DC.H, 100, 64), torch.bfloat16, lay) for lay in ("static", "bshd")]
    swas = [b.clone() for b, _ in spare]
    short = tuple(torch.zeros(DC.B, DC.H, 599, 64, dtype=torch.bfloat16, device=DEV)
                  for _ in range(2))

    def unchanged():
        torch.cuda.synchronize()
        for (kc, vc), (kw_, vw_) in zip(caches, was):
            assert torch.equal(_ints(kc[0]), _ints(kw_)) and torch.equal(_ints(vc[0]), _ints(vw_))
        for (b, _), w in zip(spare, swas):
            assert torch.equal(_ints(b), _ints(w))
        assert not short[0].any() and not short[1].any()

    # layer 1 is skipped by the method: its destination is filled by a copy after the method ran
    kw = dict(fix_kv_size=100, keep_ratio=0.25, skip_layers=[1])
    for first in ("inplace", (spare[0][1], spare[1][1])):
        with pytest.raises(ValueError, match="layer 1: K destination holds 599 rows, the result has 600"):
            fix_size_l2_compress(list(tin), out=[first, short], **kw)
        unchanged()
    with pytest.raises(ValueError, match="layer 1: V destination overlaps the layer's V"):
        fix_size_l2_compress(list(tin), out=["inplace", (torch.zeros_like(tin[1][0]),
                                                         _window(caches[1][1][0], "bshd", 600, 30))],
                             **kw)
    unchanged()

    # h2o_attention_compress with a manager: the manager is updated before the jobs exist
    rng = np.random.default_rng(15)
    Hh, S, start, hh, recent = 3, 600, 4, 64, 128
    hkw = dict(start_size=start, heavy_hitter_size=hh, recent_size=recent)
    hl = [(k[:1], v[:1]) for k, v in tin]
    mgr = HA.H2OAttentionManager(**hkw)
    att = [tuple(_tie_attention(rng, (1, Hh, 2, S)).to(torch.bfloat16).to(DEV) for _ in hl)
           for _ in range(2)]
    mgr.update_attention_scores(att[0])
    mgr2 = copy.deepcopy(mgr)
    state = (dict(mgr.accumulated_attention), mgr.current_seq_len)
    n = start + hh + recent
    bad = tuple(torch.zeros(1, Hh, n - 1, 64, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    with pytest.raises(ValueError, match="layer 1: K destination holds 195 rows, the result has 196"):
        HA.h2o_attention_compress(list(hl), attention_scores=att[1], h2o_manager=mgr,
                                  out=["inplace", bad], **hkw)
    unchanged()
    assert not bad[0].any() and not bad[1].any()
    assert mgr.current_seq_len == state[1] and set(mgr.accumulated_attention) == set(state[0])
    assert all(mgr.accumulated_attention[i] is state[0][i] for i in state[0])
    # the retry accumulates this step once: it equals the default call from the same state
    want = HA.h2o_attention_compress([(k.clone(), v.clone()) for k, v in hl],
                                     attention_scores=att[1], h2o_manager=mgr2, **hkw)
    good = [tuple(torch.zeros(1, Hh, n, 64, dtype=torch.bfloat16, device=DEV) for _ in range(2))
            for _ in hl]
    out = HA.h2o_attention_compress(list(hl), attention_scores=att[1], h2o_manager=mgr, out=good,
                                    **hkw)
    for li in range(2):
        assert torch.equal(mgr.accumulated_attention[li], mgr2.accumulated_attention[li])
        for y, w, g in zip(out[li], want[li], good[li]):
            assert y.data_ptr() == g.data_ptr() and torch.equal(_ints(y), _ints(w.contiguous()))
    unchanged()
