"""Randomised GPU parity of the delivery paths: the `out` kwarg of the compress functions (in
place, strided destinations) and compress_paged (compaction in pages, pages to dense
destinations), engine vs the CPU oracle, byte for byte.

Cases: tests/delivery_cases.py (seeded and stratified: a failure names its case; what the cases
can tell apart is shown without a GPU in tests/test_delivery_cases.py).  Every check is ONE
comparison of every buffer the call could touch -- the whole storage of every input view, every
destination cache, every page pool -- with a copy taken before the call that has the oracle's rows
written where they belong: the result, and every byte that must not change.
"""
import os

import numpy as np
import pytest
import torch

import delivery_cases as DV
import paged_util as PU
import strided_layouts as SL
from gpu_util import kind_of, to_dev, to_np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_CASES = int(os.environ.get("KVC_DELIVERY_CASES", str(DV.N_CASES)))  # more for a soak run
REFUSAL = "cannot be compacted in place"


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


class _Memory:
    """The storages a call may touch, each with the copy it is compared with afterwards."""

    def __init__(self):
        self.items = {}

    def add(self, t):
        st = t.untyped_storage()
        if st.data_ptr() not in self.items:
            flat = torch.empty(0, dtype=t.dtype, device=t.device).set_(st)
            self.items[st.data_ptr()] = (flat, flat.clone())

    def expect(self, view, rows):
        """Rows [0, n) of `view` are expected to hold `rows` (numpy [B, H, n, D])."""
        n = rows.shape[2]
        if n:
            snap = self.items[view.untyped_storage().data_ptr()][1]
            snap.as_strided(view.shape, view.stride(), view.storage_offset())[:, :, :n].copy_(
                to_dev(rows, DEV))

    def check(self, ctx):
        torch.cuda.synchronize()
        for flat, snap in self.items.values():
            assert torch.equal(PU.ints(flat), PU.ints(snap)), ctx


def _accept_refusal(c, ref, err):
    """A refused in-place compaction is right only where the oracle's row map of an in-place
    layer is not strictly increasing or its result is longer than the input."""
    assert REFUSAL in str(err), (c["case"], str(err))
    assert not isinstance(ref, Exception)
    src = DV.row_maps(c, ref)
    assert any(DV.refusable(src[li], c["layers"][li][0].shape[2]) for li in DV.inplace_layers(c)), \
        (c["case"], "refused without a reason", str(err))


def _dest(shape, dtype, layout):
    """A [B, H, S_d, D] window a few rows into a poisoned cache that is 37 rows longer, stored
    [B, H, T, D] ("static") or [B, T, H, D] ("bshd"): test_dest_gpu._dest, for B = H = 1 as well."""
    B, H, Sd, D = shape
    start = DV.DST_START[layout]
    if layout == "static":
        back = SL.new_backing("static", (B, H, Sd + DV.DST_PAD - SL.STATIC_PAD, D), dtype, DEV)
    else:
        back = SL.new_backing("bshd", (B, H, Sd + DV.DST_PAD, D), dtype, DEV).permute(0, 2, 1, 3)
    assert back.size(2) == Sd + DV.DST_PAD
    return back[:, :, start:start + Sd]


def _destinations(c, ref, mem):
    """The `out` list of a case with destinations: windows of n + 5 rows in poisoned caches."""
    entries = []
    for li, (k, v) in enumerate(c["layers"]):
        if c["no_pair"] is not None and c["no_pair"][0] == li:
            entries.append(c["no_pair"][1])
            continue
        n = k.shape[2] if isinstance(ref, Exception) else ref[li][0].shape[2]
        shape = k.shape[:2] + (n + DV.DST_EXTRA, k.shape[3])
        tdt = to_dev(k[:1, :1, :1], DEV).dtype
        pair = tuple(_dest(shape, tdt, lay) for lay in c["dst_layouts"])
        assert pair[0].stride() != pair[1].stride() or shape[1] == 1
        for t in pair:
            mem.add(t)
        entries.append(pair)
    return entries


def _check_pair(ctx, mem, got, pair, rk, rv):
    for y, win, want in ((got[0], pair[0], rk), (got[1], pair[1], rv)):
        assert y.data_ptr() == win.data_ptr() and y.stride() == win.stride(), ctx
        assert tuple(y.shape) == want.shape, ctx
        assert np.array_equal(_bytes(to_np(y)), _bytes(want)), ctx
        mem.expect(win, want)


def _run_dense(c, ref):
    from kvcompress.methods import get_compress_fn
    fn = get_compress_fn(c["method"])
    tin = [SL.make_pair(c["k_layout"], c["v_layout"], k, v, DEV) for k, v in c["layers"]]
    mem = _Memory()
    for k, v in tin:
        mem.add(k)
        mem.add(v)
    if c["path"] == "inplace":
        entries = ["inplace"] * len(tin)
        arg = "inplace"
    else:
        entries = _destinations(c, ref, mem)
        arg = list(entries)
    ctx0 = (c["case"], c["path"], c["method"], c["dtype"], c["D"], c["kw"], c["k_layout"],
            c["v_layout"])
    if isinstance(ref, Exception):
        with pytest.raises(type(ref)):
            fn(list(tin), out=arg, **c["kw"])
        mem.check(ctx0 + ("after the error",))
        return
    try:
        out = fn(list(tin), out=arg, **c["kw"])
    except ValueError as e:
        _accept_refusal(c, ref, e)
        mem.check(ctx0 + ("after the refusal",))
        return
    torch.cuda.synchronize()
    assert len(out) == len(ref)
    for li, ((ki, vi), (ko, vo), (rk, rv, kind), entry) in enumerate(zip(tin, out, ref, entries)):
        ctx = ctx0 + (li, kind, "pair" if isinstance(entry, tuple) else entry)
        if isinstance(entry, tuple):
            _check_pair(ctx, mem, (ko, vo), entry, rk, rv)
        elif entry is None:  # the default call's result: same objects, views or fresh tensors
            assert kind_of(ki, ko) == kind and kind_of(vi, vo) == kind, ctx
            assert np.array_equal(_bytes(to_np(ko)), _bytes(rk)), ctx + ("K",)
            assert np.array_equal(_bytes(to_np(vo)), _bytes(rv)), ctx + ("V",)
        elif kind == "same":
            assert out[li] is tin[li] or (ko is ki and vo is vi), ctx
        else:
            n = rk.shape[2]
            for x, y, want in ((ki, ko, rk), (vi, vo, rv)):
                assert y.data_ptr() == x.data_ptr() and y.stride() == x.stride(), ctx
                assert tuple(y.shape) == tuple(x.shape[:2]) + (n, x.shape[3]), ctx
                assert np.array_equal(_bytes(to_np(y)), _bytes(want)), ctx
                mem.expect(x, want)
    mem.check(ctx0 + ("whole buffers",))


def _run_paged(c, ref):
    from kvcompress import compress_paged
    pls = [PU.Layer(k, v, c["P"], 0, table=tab, n_pages=n_pages, table_cols=cols,
                    k_storage=c["k_storage"], v_storage=c["v_storage"])
           for (k, v), (tab, n_pages, cols) in zip(c["layers"], c["tables"])]
    snaps = [pl.snapshot() for pl in pls]
    mem = _Memory()
    kwargs = dict(c["kw"])
    entries = [None] * len(pls)
    if c["path"] == "paged_dense":
        entries = _destinations(c, ref, mem)
        kwargs["out"] = list(entries)
    ctx0 = (c["case"], c["path"], c["method"], c["dtype"], c["D"], c["kw"], c["P"],
            c["k_storage"], c["v_storage"])

    def untouched(why):
        torch.cuda.synchronize()
        for li, (pl, snap) in enumerate(zip(pls, snaps)):
            pl.assert_pools(snap, ctx0 + (li, why))
        mem.check(ctx0 + (why,))

    if isinstance(ref, Exception):
        with pytest.raises(type(ref)):
            compress_paged(c["method"], [pl.paged for pl in pls], **kwargs)
        untouched("after the error")
        return
    try:
        out = compress_paged(c["method"], [pl.paged for pl in pls], **kwargs)
    except ValueError as e:
        _accept_refusal(c, ref, e)
        untouched("after the refusal")
        return
    torch.cuda.synchronize()
    assert len(out) == len(ref)
    for li, (pl, snap, got, (rk, rv, kind), entry) in enumerate(zip(pls, snaps, out, ref, entries)):
        ctx = ctx0 + (li, kind, "pair" if isinstance(entry, tuple) else "in place")
        if isinstance(entry, tuple):  # the pool stays entirely unchanged
            _check_pair(ctx, mem, got, entry, rk, rv)
        elif kind == "same":
            assert got == pl.S, ctx
        else:
            n = rk.shape[2]
            assert got == n, ctx
            pl.expect(snap, rk, rv)
            kd, vd = pl.paged.to_dense(n)
            assert np.array_equal(_bytes(to_np(kd)), _bytes(rk)), ctx + ("to_dense K",)
            assert np.array_equal(_bytes(to_np(vd)), _bytes(rv)), ctx + ("to_dense V",)
        pl.assert_pools(snap, ctx)
    mem.check(ctx0 + ("destination caches",))


def _run(case, monkeypatch):
    from kvcompress import _engine
    from oracle import oracle
    c = DV.gen(case)
    monkeypatch.setattr(_engine, "tie_policy", c["tie"])
    monkeypatch.setattr(oracle, "TIE", c["tie"])
    _engine.call_memo.clear()
    ref = DV.reference(c)
    (_run_paged if c["path"].startswith("paged") else _run_dense)(c, ref)


@pytest.mark.parametrize("case", range(N_CASES))
def test_random_deliveries_match_oracle(case, monkeypatch):
    _run(case, monkeypatch)
