"""fp8 K/V through the compress functions: every method, both formats, both launch paths, against
fp8_util's expectation (the oracle on the bf16 upcast, bytes gathered at the kept positions) and
the reference goldens; every fused-kernel class; decode-shaped tails; strategy="random"; the
stable policy; plan cache and native replay; and what must raise before anything launches."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import fp8_gpu as G
import fp8_util as F
import phase_tables as PT
from gpu_util import kind_of
from kvcompress import _engine as E
from oracle import oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LAUNCHES = ("fused", "split")


@pytest.fixture(autouse=True)
def _fresh_memo():
    E.call_memo.clear()
    yield
    E.call_memo.clear()


def _launch(monkeypatch, launch):
    monkeypatch.setattr(E, "split_select_gather", launch == "split")


def _fn(method):
    if method == "evict_for_space":
        from kvcompress.methods.streaming_llm import evict_for_space
        return evict_for_space
    from kvcompress.methods import get_compress_fn
    return get_compress_fn(method)


def _layers(seed, fmt, lens, D=128, H=2, variant="normal"):
    ks = [F.gen_keys(seed + i, (1, H, S, D), fmt, variant) for i, S in enumerate(lens)]
    vs = [F.gen_values(seed + i, (1, H, S, D), fmt) for i, S in enumerate(lens)]
    return ks, vs


def _check(method, oracle_fn, fmt, ks, vs, kw, ctx):
    tin = [(G.dev8(k, fmt), G.dev8(v, fmt)) for k, v in zip(ks, vs)]
    out = _fn(method)(list(tin), **kw)
    torch.cuda.synchronize()
    layers = [(F.to_bf16_bits(k, fmt), None) for k in ks]
    kinds = [kind for _, _, kind in oracle_fn(
        [(kb, np.zeros(kb.shape, np.uint16)) for kb, _ in layers], **kw)]
    want = F.expected(oracle_fn, list(zip(ks, vs)), fmt, **kw)
    assert len(out) == len(want)
    for li, ((ki, vi), (ko, vo), (wk, wv), kind) in enumerate(zip(tin, out, want, kinds)):
        assert ko.dtype == vo.dtype == F.torch_dtype(fmt), ctx
        assert kind_of(ki, ko) == kind and kind_of(vi, vo) == kind, ctx + (li, kind)
        assert np.array_equal(F.to_np(ko), wk), ctx + (li, "K")
        assert np.array_equal(F.to_np(vo), wv), ctx + (li, "V")
    return out, kinds


CALLS = [(m, m, kw) for m, (_, kw) in F.ORACLE_METHODS.items()] + [
    ("evict_for_space", "evict_for_space",
     dict(num_coming=1, start_size=4, recent_size=252, skip_layers=[])),
    ("h2o_attention", "h2o_l2", F.ORACLE_METHODS["h2o_l2"][1]),  # no manager: h2o_l2's selection
]


def _oracle_fn(name):
    return oracle.evict_for_space if name == "evict_for_space" else F.ORACLE_METHODS[name][0]


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("method, oname, kw", CALLS, ids=[c[0] for c in CALLS])
def test_every_method_matches_the_upcast_oracle(method, oname, kw, fmt, launch, monkeypatch):
    _launch(monkeypatch, launch)
    ks, vs = _layers(71000, fmt, (37, 513, 1500))
    _, kinds = _check(method, _oracle_fn(oname), fmt, ks, vs, kw, (method, fmt, launch))
    if method != "recent_only":
        assert "new" in kinds


def _golden_cases():
    with open(os.path.join(HERE, "golden", "fp8_cases.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("cid", [c["id"] for c in _golden_cases()])
def test_reference_goldens(cid, launch, monkeypatch):
    _launch(monkeypatch, launch)
    c = next(x for x in _golden_cases() if x["id"] == cid)
    fmt = c["fmt"]
    ks = [F.gen_keys(L["kseed"], tuple(L["shape"]), fmt, L["variant"]) for L in c["layers"]]
    vs = [F.gen_values(L["kseed"], tuple(L["shape"]), fmt) for L in c["layers"]]
    out = _fn(c["method"])([(G.dev8(k, fmt), G.dev8(v, fmt)) for k, v in zip(ks, vs)],
                           **c["kwargs"])
    torch.cuda.synchronize()
    for (ko, vo), r in zip(out, c["layers_out"]):
        assert ko.shape[2] == r["n_out"]
        assert hashlib.sha256(F.to_np(ko).tobytes()).hexdigest() == r["k_sha"], cid
        assert hashlib.sha256(F.to_np(vo).tobytes()).hexdigest() == r["v_sha"], cid


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("D", (64, 256))
def test_fix_size_l2_other_head_dims(D, fmt, launch, monkeypatch):
    _launch(monkeypatch, launch)
    ks, vs = _layers(72000 + D, fmt, (37, 513, 1500), D=D, variant="few")
    _check("fix_size_l2", oracle.fix_size_l2_compress, fmt, ks, vs,
           F.ORACLE_METHODS["fix_size_l2"][1], (D, fmt, launch))


# one selection per kernel class (csrc/kvc.hip launch_chunk / launch_select): 512-thread LDS,
# 1024-thread LDS, global scratch with u16 positions, global scratch with u32 positions
CLASS_ZONES = (600, 12000, 40000, 70000)


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("fmt", F.FORMATS)
@pytest.mark.parametrize("Z", CLASS_ZONES)
def test_every_selection_class(Z, fmt, launch, monkeypatch):
    from kvcompress.methods import fix_size_l2_compress
    _launch(monkeypatch, launch)
    assert [PT.kernel_for(z) for z in CLASS_ZONES] == [n for _, n in PT.KERNEL_EDGES]
    D, keep, tail = 64, 300, 20
    S = Z + tail
    k8 = F.gen_keys(73000 + Z, (1, 1, S, D), fmt, "normal")
    v8 = F.gen_values(73000 + Z, (1, 1, S, D), fmt)
    kw = dict(fix_kv_size=keep + tail, keep_ratio=tail / (keep + tail), skip_layers=[])
    assert int(kw["fix_kv_size"] * kw["keep_ratio"]) == tail
    out = fix_size_l2_compress([(G.dev8(k8, fmt), G.dev8(v8, fmt))], **kw)
    torch.cuda.synchronize()
    s = PT.spec(S, zone_start=0, zone_len=Z, n_select=keep, tail_start=Z, tail_len=tail)
    wk, wv, _ = F.expected_spec(k8, v8, s, PT.ASC, PT.SORT, fmt)
    assert np.array_equal(F.to_np(out[0][0]), wk), (Z, fmt, launch, "K")
    assert np.array_equal(F.to_np(out[0][1]), wv), (Z, fmt, launch, "V")


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_decode_shaped_tails(fmt, launch, monkeypatch):
    """k = n - 1 on tie-heavy keys, and k = n - ORDER_ROWS on the "order" keys, where only
    torch.norm's eight-lane order on the upcast drops the right rows (test_fp8_cpu's power test)."""
    _launch(monkeypatch, launch)
    for S in (37, 513, 1500):
        ks, vs = _layers(74000 + S, fmt, (S,), variant="few")
        _check("fix_size_l2", oracle.fix_size_l2_compress, fmt, ks, vs,
               dict(fix_kv_size=S - 1, keep_ratio=0.0, skip_layers=[]), (S, fmt, launch))
    S = 1500
    ks = [F.gen_keys_order(9100, (1, 2, S, 128), fmt)]
    vs = [F.gen_values(9100, (1, 2, S, 128), fmt)]
    _check("fix_size_l2", oracle.fix_size_l2_compress, fmt, ks, vs,
           dict(fix_kv_size=S - F.ORDER_ROWS, keep_ratio=0.0, skip_layers=[]),
           ("order", fmt, launch))


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_random_strategy(fmt):
    from kvcompress.methods import fix_size_l2_compress
    S, H, D, fix, P = 700, 2, 128, 256, 64
    ks, vs = _layers(75000, fmt, (S,), H=H)
    torch.manual_seed(123)
    idx = torch.stack([torch.stack([torch.randperm(S - P, device=G.DEV)[:fix - P]
                                    for _ in range(H)]) for _ in range(1)])
    idx = torch.sort(idx, dim=-1)[0].cpu().numpy()
    torch.manual_seed(123)
    out = fix_size_l2_compress([(G.dev8(ks[0], fmt), G.dev8(vs[0], fmt))], fix_kv_size=fix,
                               keep_ratio=0.25, strategy="random", skip_layers=[])
    torch.cuda.synchronize()
    for got, x in ((out[0][0], ks[0]), (out[0][1], vs[0])):
        want = np.concatenate([F.take_rows(x[:, :, :S - P], idx), x[:, :, S - P:]], axis=2)
        assert np.array_equal(F.to_np(got), want)


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_stable_policy(fmt, launch, monkeypatch):
    _launch(monkeypatch, launch)
    monkeypatch.setattr(E, "tie_policy", "stable")
    monkeypatch.setattr(oracle, "TIE", "stable")
    ks, vs = _layers(76000, fmt, (513, 1500), variant="few")
    for method in ("fix_size_l2", "snapkv_lite", "h2o_l2"):
        fn, kw = F.ORACLE_METHODS[method]
        _check(method, fn, fmt, ks, vs, kw, (method, fmt, launch, "stable"))
    monkeypatch.setattr(oracle, "TIE", "reference")
    ref = F.kept_positions(oracle.fix_size_l2_compress, ks, fmt,
                           **F.ORACLE_METHODS["fix_size_l2"][1])
    monkeypatch.setattr(oracle, "TIE", "stable")
    st = F.kept_positions(oracle.fix_size_l2_compress, ks, fmt,
                          **F.ORACLE_METHODS["fix_size_l2"][1])
    assert any(not np.array_equal(a, b) for a, b in zip(ref, st))  # the policies differ here


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_repeated_call_shape_replays_natively(fmt):
    """Four calls of one shape on fresh data: the plan cache and (from the third call on) the
    native replay of csrc/kvc_host.cpp, each with the oracle's bytes."""
    fn, kw = F.ORACLE_METHODS["fix_size_l2"]
    assert E.host_module() is not None
    r0 = E.memo_stats["replayed"]
    for step in range(4):
        ks, vs = _layers(77000 + 10 * step, fmt, (600, 601, 300), variant="few")
        _check("fix_size_l2", fn, fmt, ks, vs, kw, (fmt, step))
    assert E.memo_stats["replayed"] - r0 == 2
    # the same inputs three times: identical bytes each time
    ks, vs = _layers(77100, fmt, (600, 601, 300))
    outs = []
    for _ in range(3):
        out, _ = _check("fix_size_l2", fn, fmt, ks, vs, kw, (fmt, "same inputs"))
        outs.append([(F.to_np(k), F.to_np(v)) for k, v in out])
    for o in outs[1:]:
        for (a, b), (c, d) in zip(outs[0], o):
            assert np.array_equal(a, c) and np.array_equal(b, d)


def test_status_check_stays_quiet(monkeypatch):
    monkeypatch.setattr(E, "check_status", True)
    for fmt in F.FORMATS:
        fn, kw = F.ORACLE_METHODS["snapkv_lite"]
        ks, vs = _layers(78000, fmt, (513, 1500))
        _check("snapkv_lite", fn, fmt, ks, vs, kw, (fmt, "status check"))


# ---- what must raise before anything launches ---------------------------------------------------
def test_unsupported_inputs_raise_and_touch_nothing(monkeypatch):
    from kvcompress import PagedKV
    from kvcompress.methods import (H2OAttentionManager, fix_size_l2_compress,
                                    h2o_attention_compress)
    launched = []
    for name in ("launch", "launch_dest", "launch_paged", "launch_ragged"):
        monkeypatch.setattr(E.N, name, lambda *a, _n=name, **k: launched.append(_n) or 0)
    kw = dict(fix_kv_size=64, skip_layers=[])
    S = 300

    def pair(dtype_k, dtype_v=None, D=128, device=G.DEV):
        k = torch.full((1, 2, S, D), 0x3C, dtype=torch.uint8, device=device)
        v = torch.full((1, 2, S, D), 0x3C, dtype=torch.uint8, device=device)
        return k.view(dtype_k), v.view(dtype_v or dtype_k)

    e4, e5 = torch.float8_e4m3fn, torch.float8_e5m2
    bad = [pair(torch.float8_e4m3fnuz), pair(torch.float8_e5m2fnuz), pair(torch.uint8),
           pair(torch.int8), pair(e4, e5), pair(e5, e4), pair(e4, D=80), pair(e5, D=80),
           pair(e4, device="cpu"), pair(e5, device="cpu")]
    for k, v in bad:
        with pytest.raises((TypeError, RuntimeError, ValueError)):
            fix_size_l2_compress([(k, v)], **kw)
        with pytest.raises((TypeError, RuntimeError, ValueError)):
            fix_size_l2_compress([(k, v)], out="inplace", **kw)
        assert (k.view(torch.uint8) == 0x3C).all() and (v.view(torch.uint8) == 0x3C).all()
    # a manager with fp8 K/V: TypeError, and its state does not move
    for dt in (e4, e5):
        k, v = pair(dt, D=64)
        mgr = H2OAttentionManager(start_size=4, heavy_hitter_size=16, recent_size=44)
        attn = (torch.rand(1, 2, 1, S, device=G.DEV, dtype=torch.bfloat16).softmax(-1),)
        with pytest.raises(TypeError, match="fp8"):
            h2o_attention_compress([(k, v)], attn, mgr, start_size=4, heavy_hitter_size=16,
                                   recent_size=44)
        with pytest.raises(TypeError, match="fp8"):
            h2o_attention_compress([(k, v)], None, mgr, start_size=4, heavy_hitter_size=16,
                                   recent_size=44)
        assert not mgr.accumulated_attention and mgr.current_seq_len == 0
    # pools: fnuz, raw bytes, mixed formats
    table = torch.zeros((1, 8), dtype=torch.int32, device=G.DEV)
    for dk, dv in ((torch.float8_e4m3fnuz, None), (torch.uint8, None), (e4, e5)):
        pk = torch.zeros((8, 2, 64, 128), dtype=torch.uint8, device=G.DEV)
        with pytest.raises(ValueError):
            PagedKV(pk.view(dk), pk.clone().view(dv or dk), table, 300)
    assert launched == []


# ---- kvc_debug_select_capacity: the 512-thread SELECT / fused SELECT_GATHER with a chosen capacity --
@pytest.mark.parametrize("phases", ("select", "select_gather"))
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_debug_select_capacity(fmt, phases):
    """Layer 0 (zone 1 000) fits the 1 024-position capacity: its indices / fused output are the
    oracle's on the upcast keys.  Layer 1 (zone 3 000) exceeds it: KVC_DEV_SELECT_BOUNDS in the
    call's own status word, its index rows and output rows left as they were."""
    from kvcompress import _native as N
    H, D, n_sel = 2, 128, 100
    specs = [PT.spec(S, zone_start=0, zone_len=S, n_select=n_sel) for S in (1000, 3000)]
    ks = [F.gen_keys(79000 + i, (1, H, s["S"], D), fmt, "few") for i, s in enumerate(specs)]
    vs = [F.gen_values(79000 + i, (1, H, s["S"], D), fmt) for i, s in enumerate(specs)]
    dev = [(G.dev8(k, fmt), G.dev8(v, fmt)) for k, v in zip(ks, vs)]
    outs = [tuple(torch.full((1, H, n_sel, D), F.POISON8, dtype=torch.uint8, device=G.DEV)
                  for _ in range(2)) for _ in specs]
    table = np.array([G.layer_row(s, s["S"], k, v, ko, vo)
                      for s, (k, v), (ko, vo) in zip(specs, dev, outs)], dtype=N.LAYER_DTYPE)
    L = G.Launch(G.KVC[fmt], 1, H, D, PT.ASC, PT.SORT, table, flags=N.FLAG_SPLIT_SELECT_GATHER)
    L.run(N.PHASE_SCORE)  # the norm region of both layers
    istr = int(L.info.index_row_stride)
    assert (L.indices() == -1).all()  # the 0xFF-filled workspace
    L.p.phases = N.PHASE_SELECT if phases == "select" else N.PHASE_SELECT | N.PHASE_GATHER
    rc = N.debug_select_capacity(L.p, table, L.ws.data_ptr(), int(L.info.workspace_bytes), 1024,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(L.status.item()) == N.DEV_SELECT_BOUNDS
    wk, wv, idx = F.expected_spec(ks[0], vs[0], specs[0], PT.ASC, PT.SORT, fmt)
    if phases == "select":
        got = L.indices()
        assert np.array_equal(got[:H, :n_sel], idx.reshape(H, n_sel))
        assert (got[H:] == -1).all() and istr >= n_sel
        assert all((o.cpu().numpy() == F.POISON8).all() for pair in outs for o in pair)
    else:
        assert np.array_equal(outs[0][0].cpu().numpy(), wk)
        assert np.array_equal(outs[0][1].cpu().numpy(), wv)
        assert all((o.cpu().numpy() == F.POISON8).all() for o in outs[1])
    for cap in (0, 100, 8256):  # bad capacities are refused on the host
        assert N.debug_select_capacity(L.p, table, L.ws.data_ptr(), int(L.info.workspace_bytes),
                                       cap, torch.cuda.current_stream().cuda_stream) == -1
