"""CUDA graph capture and replay of every launch path ("CUDA graphs").

Every GPU test follows one protocol: capture with torch.cuda.graph (default capture error mode)
over static inputs, static outputs and -- at the C ABI -- a static workspace; before each replay
the inputs are refilled with another seeded fill through copy_ (the pointers stay) and the
outputs reset to a sentinel; after the replay the bytes are compared with the CPU oracle's for
THAT fill.  At least two fills per case, one further replay over the workspace the replays before
it left behind, and the graph is deleted and the device synchronised at the end.

Every test that needs the GPU carries @pytest.mark.gpu itself (no module-wide pytestmark): the
unmarked tests at the end run without a GPU: the oracle's outputs for the fills of every
case differ from one another (bytes, and where the case selects the index sets too) and hold no
sentinel element, so a replay that did nothing, or that replayed old data, cannot pass.
"""
import ctypes

import numpy as np
import pytest
import torch

import dest_cases as DC
import graph_cases as GC
import phase_tables as PT
from gpu_util import kind_of, to_dev, to_np
from kvcompress import _native as N

gpu = pytest.mark.gpu

D = GC.D
DEV = "cuda:0"
INT = {2: torch.int16, 4: torch.int32}
ALL, SCORE, SELECT, GATHER = N.PHASE_ALL, N.PHASE_SCORE, N.PHASE_SELECT, N.PHASE_GATHER
# the three launch shapes of one captured call: (phases of each kvc_launch, flags)
SHAPES = {
    "all": ((ALL,), 0),  # the fused select_gather kernel where it applies
    "all-split-flag": ((ALL,), N.FLAG_SPLIT_SELECT_GATHER),
    "score-select-gather": ((SCORE, SELECT, GATHER), 0),  # three launches in one graph
}


def _refill(dst, src_np):
    """New contents through copy_: the static tensor keeps its address."""
    dst.copy_(to_dev(src_np, DEV))


def _ints(t):
    return t.view(INT[t.element_size()])


def _signed(x, bits):
    return x - (1 << bits) if x >= 1 << (bits - 1) else x


def _to_sentinel(t, dtype):
    _ints(t).fill_(_signed(PT.SENTINEL[dtype], 8 * t.element_size()))


def _same_bytes(t, want_np):
    return np.array_equal(GC.bits(to_np(t)), GC.bits(want_np))


# ==============================================================================================
# A. the C ABI on the capture stream
# ==============================================================================================
def _replay_table(key, shape, zero_host=False):
    """Capture the launches of `shape` for table `key` and replay them: fill 0 over a 0xFF
    workspace, fill 1 and fill 0 again over the workspace as the replay before left it.  Every
    layer's K and V equal phase_tables' expectation for the fill, no sentinel is left, the third
    replay reproduces the first byte for byte, the status word stays 0."""
    from test_phase_contract import Call, _bits
    c = GC.table_case(key)
    dtype, phase_list, flags = c["dtype"], *SHAPES[shape]
    host0, _ = GC.table_expected(key, 0)
    dev = [(to_dev(k, DEV), to_dev(v, DEV)) for k, v in host0]
    call = Call(c["specs"], dev, dtype, c["B"], c["H"], c["order"], c["algo"])
    call.new_workspace()
    for ph in phase_list:  # the warm-up: an eager call loads the kernels
        call.launch(ph, flags)
    torch.cuda.synchronize()
    ws_ptr, out_ptrs = call.ws.data_ptr(), [(k.data_ptr(), v.data_ptr()) for k, v in call.outs]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for ph in phase_list:
            call.launch(ph, flags)
    if zero_host:  # the table and the params travelled by value: the graph needs neither again
        call.table.view(np.uint8)[:] = 0
        ctypes.memset(ctypes.addressof(call.p), 0, ctypes.sizeof(call.p))
    call.ws.fill_(PT.POISON)  # before the first replay only
    sent = PT.SENTINEL[dtype]
    first = None
    for rep, fill in enumerate((0, 1, 0)):
        host, want = GC.table_expected(key, fill)
        for (dk, dv), (hk, hv) in zip(dev, host):
            _refill(dk, hk)
            _refill(dv, hv)
        for ko, vo in call.outs:
            _to_sentinel(ko, dtype)
            _to_sentinel(vo, dtype)
        g.replay()
        torch.cuda.synchronize()
        got = [(_bits(ko), _bits(vo)) for ko, vo in call.outs]
        for li, ((gk, gv), (wk, wv, _)) in enumerate(zip(got, want)):
            ctx = (GC.key_id(key), shape, rep, li)
            assert not (gk == sent).any() and not (gv == sent).any(), ctx + ("sentinel left",)
            assert np.array_equal(gk, GC.bits(wk)), ctx + ("K",)
            assert np.array_equal(gv, GC.bits(wv)), ctx + ("V",)
        if rep == 0:
            first = got
        elif rep == 2:
            for (gk, gv), (fk, fv) in zip(got, first):
                assert np.array_equal(gk, fk) and np.array_equal(gv, fv), "replay 3 != replay 1"
        assert int(call.status.item()) == 0, (shape, rep)
    assert call.ws.data_ptr() == ws_ptr
    assert [(k.data_ptr(), v.data_ptr()) for k, v in call.outs] == out_ptrs
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("key", GC.SPLIT_KEYS, ids=GC.key_id)
def test_a1_every_selection_kernel_replays(key, shape):
    """Longest zones 1 000 (512-thread LDS rows), 8 256 (1 024-thread LDS rows and the split-copy
    grid), 16 448 (global scratch, u16 positions) and 65 600 (u32 positions), bf16 (ASC + SORT)
    and, at the first two, fp32 (DESC + TOPK), each captured as one PHASE_ALL launch, PHASE_ALL
    with KVC_FLAG_SPLIT_SELECT_GATHER, and SCORE, SELECT, GATHER as three launches."""
    _replay_table(key, shape)


@gpu
@pytest.mark.parametrize("key", GC.SNAPKV_KEYS + GC.STABLE_KEYS, ids=GC.key_id)
def test_a2_snapkv_rows_and_stable_selection_replay(key):
    """KVC_SCORE_SNAPKV rows (SELECT reads the per-tile maxima SCORE left in the workspace) and
    KVC_ALGO_STABLE at the LDS and the global-scratch zone."""
    _replay_table(key, "all")


@gpu
@pytest.mark.parametrize("key", GC.CHUNK_KEYS, ids=GC.key_id)
def test_a3_each_node_keeps_its_own_layer_table(key):
    """65 layers: two argument chunks, so four kernel nodes whose by-value tables differ.  The
    host table and params are overwritten with zeros after the capture: a node that read host
    memory again at replay, or that shared one table with another node, fails on some layer."""
    _replay_table(key, "all", zero_host=True)


def _dest_capture(case, mode, monkeypatch):
    """A dest_cases call with `out` captured and replayed: the engine issues it as
    kvc_launch_dest on the capture stream.  Whole backing buffers are compared, as in
    tests/test_dest_gpu.py: rows [0, n) hold the oracle's bytes, every other byte is as it was."""
    from test_dest_gpu import DST_START, _dest, _filled, _method, _window
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "tie_policy", case["tie"])
    tagged = mode == "inplace"
    fn = _method(case["method"])
    masters = {}  # fill -> [((K backing, K window), (V backing, V window))]: never written again
    for fill in GC.FILLS:
        layers, _ = DC.reference(case, tagged=tagged, fill=fill)
        masters[fill] = [(_filled(k, "static"), _filled(v, "bshd")) for k, v in layers]
    static = [(_filled(k, "static"), _filled(v, "bshd")) for k, v in DC.reference(case, tagged, 0)[0]]
    tin = [(kc[1], vc[1]) for kc, vc in static]
    ref0 = DC.reference(case, tagged, 0)[1]
    if mode == "inplace":
        dst, arg = None, "inplace"
    else:
        dst = [tuple(_dest(tuple(k.shape[:2]) + (rk.shape[2] + 5, k.shape[3]), k.dtype, lay)
                     for lay in ("static", "bshd")) for (k, _), (rk, _, _) in zip(tin, ref0)]
        arg = [(kd[1], vd[1]) for kd, vd in dst]
        dst_was = [(kd[0].clone(), vd[0].clone()) for kd, vd in dst]
    fn(list(tin), out=arg, **case["kw"])  # the warm-up
    torch.cuda.synchronize()
    issued = []
    real = N.launch_dest
    monkeypatch.setattr(N, "launch_dest", lambda *a: issued.append(a[-1]) or real(*a))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        stream = torch.cuda.current_stream().cuda_stream
        out = fn(list(tin), out=arg, **case["kw"])
    monkeypatch.setattr(N, "launch_dest", real)
    assert issued and all(s == stream for s in issued), "kvc_launch_dest on the capture stream"
    for rep, fill in enumerate((0, 1, 0)):
        ref = DC.reference(case, tagged, fill)[1]
        for (kc, vc), (km, vm) in zip(static, masters[fill]):  # the pristine master of the fill
            kc[0].copy_(km[0])
            vc[0].copy_(vm[0])
        if dst is not None:
            for (kd, vd), (kw_, vw_) in zip(dst, dst_was):
                kd[0].copy_(kw_)
                vd[0].copy_(vw_)
        g.replay()
        torch.cuda.synchronize()
        for li, ((ko, vo), (rk, rv, kind)) in enumerate(zip(out, ref)):
            assert kind == "new", (case["id"], li)
            n = rk.shape[2]
            for j, (y, want, layout) in enumerate(((ko, rk, "static"), (vo, rv, "bshd"))):
                ctx = (case["id"], mode, rep, li, layout)
                assert tuple(y.shape) == want.shape and _same_bytes(y, want), ctx
                src_exp = masters[fill][li][j][0].clone()
                if mode == "inplace":
                    assert y.data_ptr() == tin[li][j].data_ptr(), ctx
                    _window(src_exp, layout, n).copy_(to_dev(want, DEV))
                else:
                    back, win = dst[li][j]
                    assert y.data_ptr() == win.data_ptr(), ctx
                    exp = dst_was[li][j].clone()
                    _window(exp, layout, n, DST_START[layout]).copy_(to_dev(want, DEV))
                    assert torch.equal(_ints(back), _ints(exp)), ctx + ("poison around the rows",)
                assert torch.equal(_ints(static[li][j][0]), _ints(src_exp)), ctx + ("cache",)
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("mode", ["inplace", "strided"])
def test_a4_destinations_replay(mode, monkeypatch):
    """The smallest selecting in-place and strided cases of tests/dest_cases.py."""
    _dest_capture(GC.DEST_INPLACE if mode == "inplace" else GC.DEST_STRIDED, mode, monkeypatch)


@gpu
def test_a5_status_word_is_set_by_every_replay_and_stays_set():
    """An external-index gather with one index behind its zone: every replay clamps it and ORs
    KVC_DEV_INDEX_RANGE into the caller's status word -- after the first replay, again after the
    word was zeroed, and still there after two replays without zeroing."""
    c = GC.STATUS
    H, S, n_sel = c["H"], c["S"], len(c["index"])
    k = torch.empty(1, H, S, D, device=DEV)
    v = torch.empty_like(k)
    ko = torch.empty(1, H, n_sel, D, device=DEV)
    vo = torch.empty_like(ko)
    t = np.zeros(1, dtype=N.LAYER_DTYPE)
    t[0] = (k.data_ptr(), v.data_ptr(), ko.data_ptr(), vo.data_ptr(), (H * S * D, S * D, D),
            (H * S * D, S * D, D), S, c["zone_start"], c["zone_len"], n_sel, 0, 0, 0, 0, 0, 0, 0,
            0, 0)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = N.Params(dtype=N.KVC_F32, batch=1, heads=H, head_dim=D, order=0, algo=0,
                 phases=GATHER, external_index=1, flags=N.FLAG_SHARED_INDEX,
                 device_status=status.data_ptr())
    rc, info = N.plan(p, t)
    assert rc == 0
    ws = torch.zeros(int(info.workspace_bytes), dtype=torch.uint8, device=DEV)
    idx = ws[info.index_offset:info.index_offset + 4 * n_sel].view(torch.int32)
    idx.copy_(torch.tensor(c["clamped"], dtype=torch.int32))
    launch = lambda: N.launch(p, t, ws.data_ptr(), int(info.workspace_bytes),  # noqa: E731
                              torch.cuda.current_stream().cuda_stream)
    _refill(k, GC.status_keys(0))
    assert launch() == 0  # the warm-up, every index inside the zone
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    idx.copy_(torch.tensor(c["index"], dtype=torch.int32))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert launch() == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0  # a capture runs nothing
    rows = torch.tensor(c["clamped"], device=DEV) + c["zone_start"]

    def replay(fill):
        kn = GC.status_keys(fill)
        _refill(k, kn)
        _refill(v, -kn)
        ko.fill_(float("nan"))
        vo.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(ko, k[:, :, rows]) and torch.equal(vo, v[:, :, rows]), fill
        return int(status.item())

    assert replay(0) == N.DEV_INDEX_RANGE
    status.zero_()
    assert replay(1) == N.DEV_INDEX_RANGE  # set again
    assert replay(2) == N.DEV_INDEX_RANGE and replay(3) == N.DEV_INDEX_RANGE  # sticky
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()


class _H2OChain:
    """Static buffers and tables of kvc_attn_accumulate -> kvc_heavy_hitters (into the index region
    of a KVC_FLAG_SHARED_INDEX plan) -> the gather, for GC.H2O."""

    def __init__(self):
        from kvcompress import _cpu_order as CO
        c = GC.H2O
        L, H, S, q = c["L"], c["H"], c["S"], c["q"]
        self.dtype = c["dtype"]
        tdt = torch.bfloat16
        m0, m = c["start"], S - c["start"] - c["recent"]
        k_sel = min(c["heavy"], m)
        n_out = c["start"] + k_sel + c["recent"]
        new = lambda *shape: torch.empty(shape, dtype=tdt, device=DEV)  # noqa: E731
        self.kv = [(new(1, H, S, D), new(1, H, S, D)) for _ in range(L)]
        self.att = [new(1, H, q, S) for _ in range(L)]
        self.acc = [new(1, H, S) for _ in range(L)]
        self.outs = [(new(1, H, n_out, D), new(1, H, n_out, D)) for _ in range(L)]
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ap = N.AttnParams(dtype=N.KVC_BF16, batch=1, heads=H, vec_bytes=CO.SUM_VEC_BYTES,
                               decay=float(np.float32(c["decay"])), flags=0,
                               device_status=self.status.data_ptr())
        self.a_table = np.zeros(L, dtype=N.ATTN_LAYER_DTYPE)
        self.hh_table = np.zeros(L, dtype=N.HH_LAYER_DTYPE)
        self.table = np.zeros(L, dtype=N.LAYER_DTYPE)
        for i in range(L):
            a, acc, (k, v), (ko, vo) = self.att[i], self.acc[i], self.kv[i], self.outs[i]
            self.a_table[i] = (a.data_ptr(), a.stride()[:3], 0, acc.data_ptr(), q, S, 0,
                               CO.attn_sum_chunk(a, 1))
            self.hh_table[i] = (acc.data_ptr(), S, m0, m, k_sel, CO.head_sum_chunk(1, H, m, 2, 1), 0)
            self.table[i] = (k.data_ptr(), v.data_ptr(), ko.data_ptr(), vo.data_ptr(),
                             k.stride()[:3], v.stride()[:3], S, m0, m, k_sel, c["start"],
                             S - c["recent"], c["recent"], 0, 0, 0, 0, 0, 0)
        self.p = self.params(0)
        rc, self.info = N.plan(self.p, self.table)
        assert rc == 0 and k_sel <= int(self.info.index_row_stride)
        rc, hh_bytes = N.hh_workspace(self.ap, self.hh_table)
        assert rc == 0
        self.hh_bytes = hh_bytes
        self.hh_ws = torch.full((max(hh_bytes, 256),), PT.POISON, dtype=torch.uint8, device=DEV)
        self.ws = torch.full((int(self.info.workspace_bytes),), PT.POISON, dtype=torch.uint8,
                             device=DEV)
        self.k_sel = k_sel

    def params(self, extra_flags):
        c = GC.H2O
        return N.Params(dtype=N.KVC_BF16, batch=1, heads=c["H"], head_dim=D, order=0, algo=0,
                        phases=GATHER, external_index=1,
                        flags=N.FLAG_SHARED_INDEX | extra_flags,
                        device_status=self.status.data_ptr())

    def accumulate(self, stream):
        assert N.attn_accumulate(self.ap, self.a_table, stream.cuda_stream) == 0

    def heavy_hitters(self, stream):
        rc = N.heavy_hitters(self.ap, self.hh_table, self.ws.data_ptr() + int(self.info.index_offset),
                             int(self.info.index_row_stride), self.hh_ws.data_ptr(), self.hh_bytes,
                             stream.cuda_stream)
        assert rc == 0

    def gather(self, p, stream):
        rc = N.launch(p, self.table, self.ws.data_ptr(), int(self.info.workspace_bytes),
                      stream.cuda_stream)
        assert rc == 0

    def poison(self):
        self.ws.fill_(PT.POISON)
        self.hh_ws.fill_(PT.POISON)

    def check_replays(self, g):
        self.poison()  # before the first replay only
        first = None
        for rep, fill in enumerate((0, 1, 0)):
            e = GC.h2o_expected(fill)
            for i in range(len(self.kv)):
                _refill(self.kv[i][0], e["layers"][i][0])
                _refill(self.kv[i][1], e["layers"][i][1])
                _refill(self.att[i], e["atts"][i])
                for t in self.outs[i] + (self.acc[i],):
                    _to_sentinel(t, self.dtype)
            g.replay()
            torch.cuda.synchronize()
            off, stride = int(self.info.index_offset), int(self.info.index_row_stride)
            idx = self.ws[off:off + 4 * len(self.kv) * stride].view(torch.int32)
            idx = idx.view(len(self.kv), stride)
            for i in range(len(self.kv)):
                ctx = (rep, i)
                assert _same_bytes(self.acc[i], e["acc"][i]), ctx + ("accumulation",)
                assert idx[i, :self.k_sel].cpu().tolist() == e["idx"][i].tolist(), ctx + ("index",)
                assert _same_bytes(self.outs[i][0], e["out"][i][0]), ctx + ("K",)
                assert _same_bytes(self.outs[i][1], e["out"][i][1]), ctx + ("V",)
            got = [(to_np(k), to_np(v)) for k, v in self.outs]
            if rep == 0:
                first = got
            elif rep == 2:
                assert all(np.array_equal(a, b) for x, y in zip(got, first) for a, b in zip(x, y))
            assert int(self.status.item()) == 0


@gpu
def test_a6_h2o_chain_on_one_stream_replays():
    """kvc_attn_accumulate, kvc_heavy_hitters into the index region of a KVC_FLAG_SHARED_INDEX
    plan and the gather, captured as one chain on the capture stream; S = 600, two layers,
    against oracle/h2o_oracle.py: accumulations, index rows and K / V of every fill."""
    ch = _H2OChain()
    cur = torch.cuda.current_stream()
    for e in [GC.h2o_expected(0)]:  # the warm-up
        for i in range(len(ch.kv)):
            _refill(ch.att[i], e["atts"][i])
    ch.accumulate(cur)
    ch.heavy_hitters(cur)
    ch.gather(ch.p, cur)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream()
        ch.accumulate(s)
        ch.heavy_hitters(s)
        ch.gather(ch.p, s)
    ch.check_replays(g)
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()


@gpu
def test_a7_h2o_chain_with_the_fixed_rows_on_a_second_stream_replays():
    """The chain of A6 in the shape of the engine's execute_shared(overlap=True): the
    KVC_FLAG_GATHER_FIXED launch (sink and recent rows) on a second stream, forked from the
    capture stream by an event and joined back by another, beside the heavy hitters and the
    KVC_FLAG_GATHER_SELECTED launch on the capture stream -- two parallel branches in the
    graph."""
    ch = _H2OChain()
    p_fixed, p_sel = ch.params(N.FLAG_GATHER_FIXED), ch.params(N.FLAG_GATHER_SELECTED)
    side = torch.cuda.Stream()
    fork, join = torch.cuda.Event(), torch.cuda.Event()

    def chain(s):
        ch.accumulate(s)
        fork.record(s)
        side.wait_event(fork)
        ch.gather(p_fixed, side)
        ch.heavy_hitters(s)
        ch.gather(p_sel, s)
        join.record(side)
        s.wait_event(join)

    e = GC.h2o_expected(0)
    for i in range(len(ch.kv)):
        _refill(ch.att[i], e["atts"][i])
    chain(torch.cuda.current_stream())  # the warm-up (creates the events, loads the kernels)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(torch.cuda.current_stream())
    ch.check_replays(g)
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()


# ==============================================================================================
# B. the Python API
# ==============================================================================================
def _fn(name):
    from kvcompress.methods import get_compress_fn
    return get_compress_fn(name)


def _static_layers(layers_np):
    return [(to_dev(k, DEV), to_dev(v, DEV)) for k, v in layers_np]


def _check_api(out, tin, ref, ctx):
    assert len(out) == len(ref)
    for li, ((ki, vi), (ko, vo), (rk, rv, kind)) in enumerate(zip(tin, out, ref)):
        assert kind_of(ki, ko) == kind and kind_of(vi, vo) == kind, ctx + (li, kind)
        assert tuple(ko.shape) == rk.shape, ctx + (li,)
        assert _same_bytes(ko, rk) and _same_bytes(vo, rv), ctx + (li,)


@gpu
def test_b1_decode_step_on_static_caches_replays():
    """fix_size_l2(fix_kv_size=512, out="inplace") on the windows [:, :, :513] of four
    [1, 4, 600, 64] caches: three eager warm-up calls on a side stream, the capture on that
    stream, three replays with different fills.  Whole caches are compared: rows [0, 512) of a
    compressed layer hold the oracle's bytes and every other byte is the fill's."""
    name, kw, lens = GC.DECODE
    fn = _fn(name)
    fills = (0, 1, 2)
    ref0 = GC.api_expected(name, kw, lens, 0)

    def cache_of(x_np):
        c = torch.empty(1, 4, 600, D, dtype=torch.bfloat16, device=DEV)
        _to_sentinel(c, "bf16")
        c[:, :, :x_np.shape[2]].copy_(to_dev(x_np, DEV))
        return c

    caches = [(cache_of(k), cache_of(v)) for k, v in ref0[0]]
    tin = [(k[:, :, :S], v[:, :, :S]) for (k, v), S in zip(caches, lens)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn(list(tin), out="inplace", **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = fn(list(tin), out="inplace", **kw)
    kinds = set()
    for rep, fill in enumerate(fills):
        layers, ref = GC.api_expected(name, kw, lens, fill)
        masters = [(cache_of(k), cache_of(v)) for k, v in layers]
        for (ck, cv), (mk, mv) in zip(caches, masters):
            ck.copy_(mk)
            cv.copy_(mv)
        g.replay()
        torch.cuda.synchronize()
        for li, ((ko, vo), (rk, rv, kind)) in enumerate(zip(out, ref)):
            kinds.add(kind)
            if kind == "same":
                assert ko is tin[li][0] and vo is tin[li][1], (rep, li)
            else:
                n = rk.shape[2]
                assert ko.data_ptr() == caches[li][0].data_ptr() and ko.shape[2] == n == 512
                assert _same_bytes(ko, rk) and _same_bytes(vo, rv), (rep, li)
                masters[li][0][:, :, :n].copy_(to_dev(rk, DEV))
                masters[li][1][:, :, :n].copy_(to_dev(rv, DEV))
            for j in range(2):
                assert torch.equal(_ints(caches[li][j]), _ints(masters[li][j])), (rep, li, j)
    assert kinds == {"same", "new"}  # skip_layers' default leaves layers 0 and 1 alone
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()


def _api_capture(ci, monkeypatch, split):
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "split_select_gather", split)
    name, kw = GC.API_CASES[ci]
    fn = _fn(name)
    layers0, _ = GC.api_expected(name, kw, GC.API_LENS, 0)
    tin = _static_layers(layers0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):  # Python path, recorded, replayed by kvc_host.run
            fn(list(tin), **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = fn(list(tin), **kw)
    launches = any(kind == "new" for _, _, kind in GC.api_expected(name, kw, GC.API_LENS, 0)[1])
    assert launches == (name != "recent_only")
    for rep, fill in enumerate((0, 1, 0)):
        layers, ref = GC.api_expected(name, kw, GC.API_LENS, fill)
        for (dk, dv), (hk, hv) in zip(tin, layers):
            _refill(dk, hk)
            _refill(dv, hv)
        for (ki, _), (ko, vo) in zip(tin, out):
            if kind_of(ki, ko) == "new":  # the graph pool's memory: reset, then rewritten
                _to_sentinel(ko, "bf16")
                _to_sentinel(vo, "bf16")
        if launches:  # recent_only only slices: its capture holds no node to replay
            g.replay()
        torch.cuda.synchronize()
        _check_api(out, tin, ref, (name, split, rep))
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("ci", range(len(GC.API_CASES)), ids=[c[0] for c in GC.API_CASES])
def test_b2_default_outputs_replay(ci, monkeypatch):
    """Each of the eight registry methods, captured after three warm-up calls on the capture
    stream (the third is a call-memo replay, so the captured call is one too): the returned
    tensors are the graph pool's memory and hold the oracle's bytes for the current fill after
    every replay; pass-through layers stay the same objects and slices stay views."""
    _api_capture(ci, monkeypatch, False)


@gpu
def test_b2_default_outputs_replay_with_split_select_gather(monkeypatch):
    _api_capture(1, monkeypatch, True)


def _cached_workspaces(_engine):
    plans = {e[0][2].data_ptr() for e in _engine.plan_cache.entries.values()}
    memos = {e[0].ws.data_ptr() for e in _engine.call_memo.entries.values()
             if e[0].ws is not None}
    return plans, memos


@gpu
@pytest.mark.parametrize("path", ["call-memo", "plan-cache"])
def test_b3_a_captured_call_owns_its_workspace(path, monkeypatch):
    """Warm-up calls on stream s leave the shape's workspaces in plan_cache and call_memo.  The
    capture on s must hand the launch none of them (call-memo: the capture is a kvc_host.run
    replay; plan-cache: the memo is empty and the capture hits the plan cache) and must add no
    cache entry.  Only after these pointer checks: both caches are cleared, eager calls of the
    shape run on s, the graph replays on ANOTHER stream, and both give the oracle's bytes."""
    from kvcompress import _engine
    name, kw, lens = GC.OWNED
    fn = _fn(name)
    _engine.plan_cache.clear()
    _engine.call_memo.clear()
    layers0, _ = GC.api_expected(name, kw, lens, 0)
    tin = _static_layers(layers0)
    s, other = torch.cuda.Stream(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn(list(tin), **kw)
    torch.cuda.synchronize()
    hm = _engine.host_module()
    assert hm is not None
    plans, memos = _cached_workspaces(_engine)
    assert plans and memos, "the warm-up cached the shape in both caches"
    if path == "plan-cache":
        _engine.call_memo.clear()
    held = plans | memos
    entries = (len(_engine.plan_cache.entries), len(_engine.call_memo.entries))

    seen = []  # workspace pointers handed to a launch during the capture
    real = (N.launch, N.launch_dest, hm.run)
    monkeypatch.setattr(N, "launch", lambda p, t, ws, n, st: seen.append(ws) or real[0](p, t, ws, n, st))
    monkeypatch.setattr(N, "launch_dest",
                        lambda p, t, d, ws, n, st: seen.append(ws) or real[1](p, t, d, ws, n, st))
    monkeypatch.setattr(hm, "run", lambda *a: seen.append(a[6]) or real[2](*a))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = fn(list(tin), **kw)
    monkeypatch.setattr(N, "launch", real[0])
    monkeypatch.setattr(N, "launch_dest", real[1])
    monkeypatch.setattr(hm, "run", real[2])

    # ---- before any replay ----
    assert seen, "the capture launched"
    assert not set(seen) & held, "a cached workspace was captured into the graph"
    plans2, memos2 = _cached_workspaces(_engine)
    assert not set(seen) & (plans2 | memos2), "the capture cached the graph's workspace"
    assert (len(_engine.plan_cache.entries), len(_engine.call_memo.entries)) == entries

    # ---- behaviour ----
    _engine.plan_cache.clear()
    _engine.call_memo.clear()
    for rep, fill in enumerate((1, 0)):
        layers, ref = GC.api_expected(name, kw, lens, fill)
        e_layers, e_ref = GC.api_expected(name, kw, lens, fill + 2)
        e_in = _static_layers(e_layers)
        for (dk, dv), (hk, hv) in zip(tin, layers):
            _refill(dk, hk)
            _refill(dv, hv)
        for ko, vo in out:
            _to_sentinel(ko, "bf16")
            _to_sentinel(vo, "bf16")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):  # eager calls of the shape refill the caches ...
            for _ in range(3):
                e_out = fn(list(e_in), **kw)
        with torch.cuda.stream(other):  # ... while the graph runs beside them
            g.replay()
        torch.cuda.synchronize()
        _check_api(out, tin, ref, (path, "replay", rep))
        _check_api(e_out, e_in, e_ref, (path, "eager", rep))
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()


@gpu
def test_b4_first_use_inside_a_capture_is_refused(monkeypatch):
    """The per-device status word and the side stream are made on first use.  Inside a capture
    the word would be graph-pool memory that every replay zeroes again, so the first engine call
    of a process must be eager: inside a capture it raises RuntimeError before anything is
    enqueued, makes no word, and the same capture works once an eager call has been made."""
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "_status_words", {})
    monkeypatch.setattr(_engine, "_side", {})
    _engine.plan_cache.clear()  # cached plans carry the address of the word they were made with
    _engine.call_memo.clear()
    try:
        name, kw = GC.API_CASES[1]
        fn = _fn(name)
        layers, ref = GC.api_expected(name, kw, GC.API_LENS, 0)
        tin = _static_layers(layers)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="first engine call on cuda:0 came inside a CUDA graph"):
            with torch.cuda.graph(g):
                fn(list(tin), **kw)
        assert _engine._status_words == {} and _engine._side == {}
        del g
        fn(list(tin), **kw)  # the warm-up makes the word
        torch.cuda.synchronize()
        assert list(_engine._status_words) == [0]
        g = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="side stream"):
            with torch.cuda.graph(g):
                _engine.side_stream(0)
        assert _engine._side == {}
        del g
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn(list(tin), **kw)
        g.replay()
        torch.cuda.synchronize()
        _check_api(out, tin, ref, ("after the warm-up",))
        assert _engine.device_status(0) == 0  # readable afterwards: not the graph pool's memory
        del g  # the graph goes before the test ends, and the device is idle
        torch.cuda.synchronize()
    finally:  # no plan made with this test's word outlives it
        _engine.plan_cache.clear()
        _engine.call_memo.clear()


@gpu
def test_b5_status_check_reads_nothing_while_capturing(monkeypatch):
    """With the per-call status check on, a captured call does not read the word (the read
    synchronises, which a capture forbids) and so does not raise; the first eager call after it
    reads the word as usual."""
    from kvcompress import _engine
    name, kw = GC.API_CASES[1]
    fn = _fn(name)
    layers, ref = GC.api_expected(name, kw, GC.API_LENS, 0)
    tin = _static_layers(layers)
    fn(list(tin), **kw)
    torch.cuda.synchronize()
    reads = []
    real = _engine.raise_on_status
    monkeypatch.setattr(_engine, "raise_on_status", lambda d=None: reads.append(set(d)) or real(d))
    prev = _engine.set_status_check(True)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn(list(tin), **kw)
        assert reads == []
        g.replay()
        torch.cuda.synchronize()
        _check_api(out, tin, ref, ("checked capture",))
        assert reads == []
        fn(list(tin), **kw)
        assert reads == [{0}]
    finally:
        _engine.set_status_check(prev)
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()


# ==============================================================================================
# CPU proofs (no GPU): the fills of every case tell a stale or absent replay from a real one
# ==============================================================================================
def _differ(a, b):
    return a.shape != b.shape or not np.array_equal(GC.bits(a), GC.bits(b))


def _no_sentinel(a, dtype):
    return not (GC.bits(a) == PT.SENTINEL[dtype]).any()


@pytest.mark.parametrize("key", GC.TABLE_KEYS, ids=GC.key_id)
def test_fills_of_a_table_differ(key):
    """Per layer: K and V of fill 0 and fill 1 differ and hold no sentinel element, and where the
    layer selects, so do the selected index sets of every (batch, head) row."""
    c = GC.table_case(key)
    (_, w0), (_, w1) = (GC.table_expected(key, f) for f in GC.FILLS)
    assert any(GC.selects(s) for s in c["specs"])
    for s, (k0, v0, i0), (k1, v1, i1) in zip(c["specs"], w0, w1):
        assert _differ(k0, k1) and _differ(v0, v1), s
        assert all(_no_sentinel(x, c["dtype"]) for x in (k0, v0, k1, v1)), s
        if GC.selects(s):
            rows = (i0 != i1).any(axis=-1)
            if s["variant"] == "special+scaled":
                # batch 0 of a snapkv table's last layer keeps the NaN / inf keys: one NaN norm
                # makes every snapkv score of the row NaN (phase_tables.split_table), so its
                # selection is decided by position alone, whatever the fill; its bytes differ
                rows = rows[1:]
            assert rows.all(), s


@pytest.mark.parametrize("case", [GC.DEST_INPLACE, GC.DEST_STRIDED], ids=lambda c: c["id"])
def test_fills_of_a_destination_case_differ(case):
    """The destination cases select, and the fills' selections differ: V of the in-place case
    carries its row's position, so its oracle output IS the selected set."""
    assert case in DC.INPLACE and (case is GC.DEST_INPLACE or case in DC.STRIDED)
    for tagged in (True, False):
        r0, r1 = (DC.reference(case, tagged=tagged, fill=f)[1] for f in GC.FILLS)
        for (k0, v0, kind), (k1, v1, _) in zip(r0, r1):
            assert kind == "new" and _differ(k0, k1)
            assert _no_sentinel(k0, case["dtype"]) and _no_sentinel(k1, case["dtype"])
            assert _differ(v0, v1)  # tagged: the kept positions; else the values
            if tagged:
                assert (DC.row_map(case, v0) != DC.row_map(case, v1)).any(axis=-1).all()


def test_fills_of_the_status_case_differ():
    c = GC.STATUS
    k = [GC.status_keys(f) for f in range(4)]
    rows = np.array(c["clamped"]) + c["zone_start"]
    assert c["index"][-1] == c["zone_len"] and c["clamped"][-1] == c["zone_len"] - 1
    for a in range(4):
        assert not np.isnan(k[a]).any() and float(k[a].max()) < 2 ** 24  # exact integers
        for b in range(a):
            assert _differ(k[a][:, :, rows], k[b][:, :, rows])


def test_fills_of_the_h2o_chain_differ():
    e0, e1 = (GC.h2o_expected(f) for f in GC.FILLS)
    c = GC.H2O
    for li in range(c["L"]):
        assert len(e0["idx"][li]) == c["heavy"] and (e0["idx"][li] != e1["idx"][li]).any()
        assert _differ(e0["acc"][li], e1["acc"][li])
        for j in range(2):
            assert _differ(e0["out"][li][j], e1["out"][li][j])
            assert _no_sentinel(e0["out"][li][j], c["dtype"])
            assert _no_sentinel(e1["out"][li][j], c["dtype"])
        assert _no_sentinel(e0["acc"][li], c["dtype"]) and _no_sentinel(e1["acc"][li], c["dtype"])


def _api_proof(name, kw, lens, fills):
    refs = [GC.api_expected(name, kw, lens, f)[1] for f in fills]
    assert any(kind == "new" for _, _, kind in refs[0]) or name == "recent_only"
    for a in range(len(refs)):
        for k, v, kind in refs[a]:
            assert _no_sentinel(k, "bf16") and _no_sentinel(v, "bf16")
        for b in range(a):
            assert [x[2] for x in refs[a]] == [x[2] for x in refs[b]]
            for (k0, v0, _), (k1, v1, _) in zip(refs[a], refs[b]):
                assert _differ(k0, k1) and _differ(v0, v1), (name, a, b)


@pytest.mark.parametrize("ci", range(len(GC.API_CASES)), ids=[c[0] for c in GC.API_CASES])
def test_fills_of_an_api_case_differ(ci):
    _api_proof(*GC.API_CASES[ci], GC.API_LENS, GC.FILLS)


def test_fills_of_the_decode_and_owned_cases_differ():
    _api_proof(*GC.DECODE, (0, 1, 2))
    _api_proof(*GC.OWNED, (0, 1, 2, 3))


def test_first_use_inside_a_capture_is_refused_before_anything_is_made(monkeypatch):
    """The host logic of B4 without a device: while the current stream is capturing, neither the
    status word nor the side stream of a device that has none yet is created."""
    from kvcompress import _engine
    monkeypatch.setattr(_engine, "_status_words", {})
    monkeypatch.setattr(_engine, "_side", {})
    monkeypatch.setattr(_engine.torch.cuda, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(_engine, "_new_status_word", lambda device: pytest.fail("a word was made"))
    with pytest.raises(RuntimeError, match="first engine call on cuda:3 came inside a CUDA graph"):
        _engine.status_word(3)
    with pytest.raises(RuntimeError, match="side stream"):
        _engine.side_stream(3)
    assert _engine._status_words == {} and _engine._side == {}
