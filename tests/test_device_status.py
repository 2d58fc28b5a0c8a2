"""The device status channel as a contract (include/kvc.h, kvc_device_status).

KVC_DEV_SELECT_BOUNDS is raised by the selection kernels when a row's zone is longer than the
kernel's capacity (csrc/kvc_select.h select_body): the row then selects nothing and -- in the fused
SELECT_GATHER kernel -- writes no output row.  kvc_launch always dispatches a sufficient capacity,
so the guard is driven through kvc_debug_select_capacity, which launches the same kernels with a
caller-chosen capacity.  (tests/conftest.py also asserts after every GPU test that the engine's
own status word stayed 0.)  Reference of the selection being guarded: fix_size_l2.py:104-108."""
import numpy as np
import pytest
import torch

from kvcompress import _native as N

pytestmark = pytest.mark.gpu
KVC_E_ARG = -1


def _table(layers, H, D):
    t = np.zeros(len(layers), dtype=N.LAYER_DTYPE)
    for i, (k, v, ko, vo, S, n_sel) in enumerate(layers):
        t[i] = (k.data_ptr(), v.data_ptr(), ko.data_ptr(), vo.data_ptr(), (H * S * D, S * D, D),
                (H * S * D, S * D, D), S, 0, S, n_sel, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    return t


@pytest.mark.parametrize("phases", ["select", "select_gather"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_select_bounds_reported_and_row_left_unwritten(phases, dt):
    H, D, n_sel = 4, 64, 100
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    specs = []
    for S in (1000, 3000):  # layer 1 exceeds the 1 024-position capacity given below
        k = torch.randn(1, H, S, D, device=dev, generator=g).to(dt)
        v = torch.randn(1, H, S, D, device=dev, generator=g).to(dt)
        ko = torch.full((1, H, n_sel, D), -7.0, device=dev, dtype=dt)
        vo = torch.full_like(ko, -7.0)
        specs.append((k, v, ko, vo, S, n_sel))
    t = _table(specs, H, D)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    dtype = {torch.bfloat16: N.KVC_BF16, torch.float32: N.KVC_F32}[dt]
    p = N.Params(dtype=dtype, batch=1, heads=H, head_dim=D, order=N.KVC_ASC,
                 algo=N.KVC_ALGO_SORT, phases=N.PHASE_ALL, external_index=0,
                 flags=N.FLAG_SPLIT_SELECT_GATHER, device_status=status.data_ptr())
    rc, info = N.plan(p, t)
    assert rc == 0
    stream = torch.cuda.current_stream().cuda_stream
    ws = torch.zeros(int(info.workspace_bytes), dtype=torch.uint8, device=dev)
    # the expected result through the normal launch (three kernels: the index region is
    # written), for layer 0
    assert N.launch(p, t, ws.data_ptr(), int(info.workspace_bytes), stream) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    rows = int(info.rows)
    istride = int(info.index_row_stride)
    iv = ws[info.index_offset:info.index_offset + rows * istride * 4].view(torch.int32)
    want_idx = iv[:H * istride].clone()
    want_k0, want_v0 = specs[0][2].clone(), specs[0][3].clone()
    for s in specs:  # sentinels in the outputs and the index region
        s[2].fill_(-7.0)
        s[3].fill_(-7.0)
    iv.fill_(-1)
    p.phases = N.PHASE_SELECT if phases == "select" else N.PHASE_SELECT | N.PHASE_GATHER
    assert N.debug_select_capacity(p, t, ws.data_ptr(), int(info.workspace_bytes), 1024,
                                   stream) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == N.DEV_SELECT_BOUNDS
    iv2 = iv.view(rows, istride)
    if phases == "select":
        # layer 0 selected exactly as the normal launch; layer 1's rows untouched
        assert torch.equal(iv2[:H, :n_sel].flatten(),
                           want_idx.view(H, istride)[:, :n_sel].flatten())
        assert bool((iv2[H:] == -1).all())
    else:
        assert torch.equal(specs[0][2], want_k0) and torch.equal(specs[0][3], want_v0)
        assert bool((specs[1][2] == -7.0).all()) and bool((specs[1][3] == -7.0).all())
    # bad capacities are refused on the host
    for cap in (0, 100, 8256):
        assert N.debug_select_capacity(p, t, ws.data_ptr(), int(info.workspace_bytes), cap,
                                       stream) == KVC_E_ARG


def test_opt_in_status_check_raises_naming_the_bit():
    """kvcompress._engine.set_status_check(True) (or KVC_CHECK_STATUS=1 at import): a compress
    call after which the engine's device word is non-zero raises RuntimeError naming the bit and
    clears the word; clean calls pass.  The bit is set through kvc_debug_select_capacity on the
    engine's own word, as a dispatch bug inside a call would set it."""
    from kvcompress import _engine as E
    from kvcompress.methods import fix_size_l2_compress
    H, D, n_sel, S = 4, 64, 100, 3000
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(9)
    k = torch.randn(1, H, S, D, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(1, H, S, D, device=dev, generator=g).to(torch.bfloat16)
    ko, vo = torch.empty(1, H, n_sel, D, device=dev, dtype=k.dtype), torch.empty(
        1, H, n_sel, D, device=dev, dtype=k.dtype)
    t = _table([(k, v, ko, vo, S, n_sel)], H, D)
    word = E.status_word(0)
    p = N.Params(dtype=N.KVC_BF16, batch=1, heads=H, head_dim=D, order=N.KVC_ASC,
                 algo=N.KVC_ALGO_SORT, phases=N.PHASE_SELECT | N.PHASE_GATHER, external_index=0,
                 flags=0, device_status=word.data_ptr())
    rc, info = N.plan(p, t)
    assert rc == 0
    ws = torch.zeros(int(info.workspace_bytes), dtype=torch.uint8, device=dev)
    prev = E.set_status_check(True)
    try:
        layers = [(k, v)]
        out = fix_size_l2_compress(layers, fix_kv_size=512, skip_layers=[])  # clean: no raise
        assert out[0][0].shape[2] == 512
        assert N.debug_select_capacity(p, t, ws.data_ptr(), int(info.workspace_bytes), 1024,
                                       torch.cuda.current_stream().cuda_stream) == 0
        with pytest.raises(RuntimeError, match="KVC_DEV_SELECT_BOUNDS"):
            fix_size_l2_compress(layers, fix_kv_size=512, skip_layers=[])
        assert E.device_status(0) == 0  # cleared by the raise
        fix_size_l2_compress(layers, fix_kv_size=512, skip_layers=[])
    finally:
        E.set_status_check(prev)


class _Flagger:
    """Sets KVC_DEV_SELECT_BOUNDS on the engine's own word of cuda:0, as a dispatch bug inside a
    call would: kvc_debug_select_capacity with a capacity below the table's zone."""

    def __init__(self):
        from kvcompress import _engine as E
        H, D, n_sel, S = 4, 64, 100, 3000
        dev = torch.device("cuda:0")
        k = torch.zeros(1, H, S, D, device=dev, dtype=torch.bfloat16)
        ko = torch.empty(1, H, n_sel, D, device=dev, dtype=k.dtype)
        self.keep = (k, ko)
        self.t = _table([(k, k, ko, ko, S, n_sel)], H, D)
        self.p = N.Params(dtype=N.KVC_BF16, batch=1, heads=H, head_dim=D, order=N.KVC_ASC,
                          algo=N.KVC_ALGO_SORT, phases=N.PHASE_SELECT | N.PHASE_GATHER,
                          external_index=0, flags=0, device_status=E.status_word(0).data_ptr())
        rc, info = N.plan(self.p, self.t)
        assert rc == 0
        self.nbytes = int(info.workspace_bytes)
        self.ws = torch.zeros(self.nbytes, dtype=torch.uint8, device=dev)

    def __call__(self):
        assert N.debug_select_capacity(self.p, self.t, self.ws.data_ptr(), self.nbytes, 1024,
                                       torch.cuda.current_stream().cuda_stream) == 0


def _fix_size_entry():
    from kvcompress import _engine as E
    from kvcompress.methods import fix_size_l2_compress
    g = torch.Generator(device="cuda:0").manual_seed(21)
    layers = [tuple(torch.randn(1, 4, 3000, 64, device="cuda:0", generator=g).to(torch.bfloat16)
                    for _ in range(2)) for _ in range(2)]
    E.call_memo.clear()
    E.plan_cache.clear()
    r0 = E.memo_stats["replayed"]
    call = lambda step: fix_size_l2_compress(list(layers), fix_kv_size=512,  # noqa: E731
                                             skip_layers=[])
    return call, lambda: E.memo_stats["replayed"] - r0, 4


def _h2o_plain_entry():
    """Manager-less h2o_attention_compress: the engine's own selection through _run_plain, its
    plan cached on the second sighting and hit from the third call on."""
    from kvcompress import _engine as E
    from kvcompress.methods.h2o_attention import h2o_attention_compress
    g = torch.Generator(device="cuda:0").manual_seed(22)
    layers = [tuple(torch.randn(1, 4, 120, 64, device="cuda:0", generator=g).to(torch.bfloat16)
                    for _ in range(2)) for _ in range(2)]
    E.plan_cache.clear()
    hits = [0]
    get = E.plan_cache.get

    def counting_get(key):
        e = get(key)
        hits[0] += e is not None
        return e
    E.plan_cache.get = counting_get
    call = lambda step: h2o_attention_compress(list(layers), start_size=4,  # noqa: E731
                                               heavy_hitter_size=16, recent_size=40)

    def undo():
        del E.plan_cache.get  # the instance attribute: the class's method shows again
    return call, lambda: hits[0], 4, undo


def _h2o_manager_entry():
    """Decode steps with a manager: the first two take the Python path (two accumulation
    shapes), the rest are replayed by kvc_host.run_h2o."""
    from kvcompress.methods import h2o_attention as HA
    g = torch.Generator(device="cuda:0").manual_seed(23)
    S = 120
    layers = [tuple(torch.randn(1, 4, S, 64, device="cuda:0", generator=g).to(torch.bfloat16)
                    for _ in range(2)) for _ in range(2)]
    atts = [tuple(torch.rand(1, 4, 1, S, device="cuda:0", generator=g).to(torch.bfloat16)
                  for _ in range(2)) for _ in range(6)]
    mgr = HA.H2OAttentionManager(start_size=4, heavy_hitter_size=16, recent_size=40)
    HA.step_memo.clear()
    r0 = HA.step_stats["replayed"]
    call = lambda step: HA.h2o_attention_compress(  # noqa: E731
        list(layers), attention_scores=atts[step], h2o_manager=mgr, start_size=4,
        heavy_hitter_size=16, recent_size=40)
    return call, lambda: HA.step_stats["replayed"] - r0, 5


@pytest.mark.parametrize("flagged", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("entry", [_fix_size_entry, _h2o_plain_entry, _h2o_manager_entry],
                         ids=["fix_size_l2", "h2o_attention-no-manager", "h2o_attention-manager"])
def test_status_is_read_after_cached_and_replayed_calls(entry, flagged):
    """With the check on, the word is read after EVERY call: of five consecutive same-shape calls
    -- the later ones served by the plan cache, the call memo's native replay or the native
    decode-step replay -- exactly the one a bit was set before raises, naming the bit; the word
    is clear afterwards and the next call passes.  The entry point must have reached its cached /
    replayed path within the five calls (by the fourth for the call memo)."""
    from kvcompress import _engine as E
    call, replayed, by, *undo = entry()
    flag = _Flagger()
    prev = E.set_status_check(True)
    raised = []
    try:
        for i in range(1, 6):
            if i == flagged:
                flag()
            try:
                out = call(i - 1)
                assert out[0][0].shape[2] < 3000
            except RuntimeError as e:
                assert "KVC_DEV_SELECT_BOUNDS" in str(e)
                raised.append(i)
                assert E.device_status(0) == 0  # cleared by the raise
            if i == by:
                assert replayed() > 0, "the cached / replayed path was never taken"
        call(5)  # the next call passes
        assert raised == [flagged]
    finally:
        E.set_status_check(prev)
        for u in undo:
            u()
        E.device_status(0, clear=True)  # a failure above must not be blamed on the next test


def _external_gather(dt, flags, idx_rows, outs=None, shared=False):
    """GATHER of one [1, 4, 256, 64] layer (sink 2, zone (10, 100), 3 selected, tail (200, 3))
    through caller-written index rows; returns (k, v, ko, vo, status bits)."""
    H, S, D, n_sel, sink, tail = 4, 256, 64, 3, 2, 3
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(31)
    k = torch.randn(1, H, S, D, device=dev, generator=g).to(dt)
    v = torch.randn(1, H, S, D, device=dev, generator=g).to(dt)
    if outs is None:
        outs = tuple(torch.full((1, H, sink + n_sel + tail, D), -7.0, device=dev, dtype=dt)
                     for _ in range(2))
    ko, vo = outs
    t = np.zeros(1, dtype=N.LAYER_DTYPE)
    t[0] = (k.data_ptr(), v.data_ptr(), ko.data_ptr(), vo.data_ptr(), (H * S * D, S * D, D),
            (H * S * D, S * D, D), S, 10, 100, n_sel, sink, 200, tail, 0, 0, 0, 0, 0, 0)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    p = N.Params(dtype={torch.bfloat16: N.KVC_BF16, torch.float32: N.KVC_F32}[dt], batch=1,
                 heads=H, head_dim=D, order=0, algo=0, phases=N.PHASE_GATHER, external_index=1,
                 flags=flags, device_status=status.data_ptr())
    rc, info = N.plan(p, t)
    assert rc == 0
    ws = torch.full((int(info.workspace_bytes),), 0xFF, dtype=torch.uint8, device=dev)
    rows, istride = int(info.rows), int(info.index_row_stride)
    assert rows == H
    iv = ws[info.index_offset:info.index_offset + rows * istride * 4].view(torch.int32)
    iv = iv.view(rows, istride)
    iv[:len(idx_rows), :n_sel] = torch.tensor(idx_rows, dtype=torch.int32)
    assert N.launch(p, t, ws.data_ptr(), int(info.workspace_bytes),
                    torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return k, v, ko, vo, int(status.item())


# per-head rows: head 1 holds a negative index, head 2 one equal to zone_len
_BAD_ROWS = [[5, 7, 99], [-1, 7, 99], [5, 7, 100], [0, 50, 99]]
_CLAMPED = [[5, 7, 99], [0, 7, 99], [5, 7, 99], [0, 50, 99]]


def _want(x, rows):
    src = torch.tensor([[0, 1] + [10 + i for i in r] + [200, 201, 202] for r in rows],
                       device=x.device)
    return x[0].gather(1, src[:, :, None].expand(-1, -1, x.shape[3]))[None]


def _eq(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_index_range_reported_per_head(dt):
    """KVC_DEV_INDEX_RANGE without KVC_FLAG_SHARED_INDEX: every head reads its own index row; a
    negative index is clamped to the zone's first row, one equal to zone_len to its last, the bit
    is reported, and the heads with in-range indices are exact.  In-range rows report nothing."""
    k, v, ko, vo, bits = _external_gather(dt, 0, _CLAMPED)
    assert bits == 0
    assert _eq(ko, _want(k, _CLAMPED)) and _eq(vo, _want(v, _CLAMPED))
    k, v, ko, vo, bits = _external_gather(dt, 0, _BAD_ROWS)
    assert bits == N.DEV_INDEX_RANGE
    assert _eq(ko, _want(k, _CLAMPED)) and _eq(vo, _want(v, _CLAMPED))
    assert _eq(ko[0, 1, 2], k[0, 1, 10]) and _eq(ko[0, 2, 4], k[0, 2, 109])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_index_range_in_the_two_launch_copy(dt):
    """The copy in two launches over the same bad indices: KVC_FLAG_GATHER_FIXED never reads an
    index (word 0; sink and tail rows only, the sentinel survives in the selected rows),
    KVC_FLAG_GATHER_SELECTED clamps and reports (selected rows only); into one pair of outputs
    the two equal the one-launch copy."""
    k, v, ko1, vo1, bits = _external_gather(dt, 0, _BAD_ROWS)
    assert bits == N.DEV_INDEX_RANGE
    sel = slice(2, 5)
    _, _, kof, vof, bits = _external_gather(dt, N.FLAG_GATHER_FIXED, _BAD_ROWS)
    assert bits == 0
    for of, o1 in ((kof, ko1), (vof, vo1)):
        assert bool((of[:, :, sel] == -7.0).all())
        assert _eq(of[:, :, :2], o1[:, :, :2]) and _eq(of[:, :, 5:], o1[:, :, 5:])
    _, _, kos, vos, bits = _external_gather(dt, N.FLAG_GATHER_SELECTED, _BAD_ROWS)
    assert bits == N.DEV_INDEX_RANGE
    for os_, o1 in ((kos, ko1), (vos, vo1)):
        assert bool((os_[:, :, :2] == -7.0).all()) and bool((os_[:, :, 5:] == -7.0).all())
        assert _eq(os_[:, :, sel], o1[:, :, sel])
    _, _, ko2, vo2, bits = _external_gather(dt, N.FLAG_GATHER_SELECTED, _BAD_ROWS, (kof, vof))
    assert bits == N.DEV_INDEX_RANGE
    assert _eq(ko2, ko1) and _eq(vo2, vo1)


def test_status_word_first_made_inside_inference_mode_stays_clearable():
    """The evaluation loops run under torch.inference_mode(); a status word first created there
    must still be a normal tensor, which device_status(clear=True) zeroes in place afterwards."""
    from kvcompress import _engine as E
    with torch.inference_mode():
        w = E._new_status_word(0)
    assert not w.is_inference()
    w.zero_()
    torch.cuda.synchronize()
    assert int(w.item()) == 0
