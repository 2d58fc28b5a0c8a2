"""The C ABI's phase contract (include/kvc.h, "Phases"): SCORE, SELECT and GATHER launched one
at a time on one workspace produce the bytes of one KVC_PHASE_ALL launch, no phase reads a
workspace byte that an earlier phase of the call did not write, and SELECT of plain-norm rows
depends on columns [0, zone_len) of the norm region alone.

Every workspace here starts as 0xFF bytes (NaN as a norm, -1 as an index) and every output as a
sentinel; the expectations are built on the CPU from the oracle's primitives
(tests/phase_tables.py, proved against the oracle's methods in tests/test_phase_tables.py).  All
comparisons are on bytes.

Which selection kernel each longest zone reaches (csrc/kvc.hip launch_select): 1 000 the
512-thread LDS rows, 8 256 the 1 024-thread LDS rows, 16 448 the global-scratch rows with u16
positions, 65 600 the u32-position rows."""
import numpy as np
import pytest
import torch

import phase_tables as PT
from gpu_util import to_dev
from kvcompress import _native as N

pytestmark = pytest.mark.gpu

D = 64
DT = {"bf16": N.KVC_BF16, "fp16": N.KVC_F16, "fp32": N.KVC_F32}
INT = {2: torch.int16, 4: torch.int32}
ALL, SCORE, SELECT, GATHER = N.PHASE_ALL, N.PHASE_SCORE, N.PHASE_SELECT, N.PHASE_GATHER
# launch shapes of one call: (phases of each kvc_launch, flags)
SHAPES = {
    "all": ((ALL,), 0),
    "score|select+gather": ((SCORE, SELECT | GATHER), 0),  # what bench.py --full's split timer issues
    "score|select|gather": ((SCORE, SELECT, GATHER), 0),
    "all, split flag": ((ALL,), N.FLAG_SPLIT_SELECT_GATHER),
}


def _signed(x, bits):
    return x - (1 << bits) if x >= 1 << (bits - 1) else x


def _bits(t):
    """A device tensor's elements as same-width integers, on the CPU."""
    return t.view(INT[t.element_size()]).cpu().numpy().view(
        {2: np.uint16, 4: np.uint32}[t.element_size()])


class Call:
    """One planned call over device inputs: fresh outputs and a fresh poisoned workspace per
    run(), one status word for all of them."""

    def __init__(self, specs, dev_layers, dtype, B, H, order, algo, flags=0, external=False):
        self.specs, self.dtype, self.B, self.H = specs, dtype, B, H
        self.layers = dev_layers
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        self.p = N.Params(dtype=DT[dtype], batch=B, heads=H, head_dim=D, order=order, algo=algo,
                          phases=GATHER if external else ALL, external_index=int(external),
                          flags=flags, device_status=self.status.data_ptr())
        self.table = np.zeros(len(specs), dtype=N.LAYER_DTYPE)
        for t, s, (k, v) in zip(self.table, specs, dev_layers):
            assert k.shape == (B, H, s["S"], D) and k.is_contiguous() and v.is_contiguous()
            t["k"], t["v"] = k.data_ptr(), v.data_ptr()
            t["k_stride"] = t["v_stride"] = k.stride()[:3]
            t["seq_len"], t["zone_start"], t["zone_len"] = s["S"], s["zone_start"], s["zone_len"]
            t["n_select"], t["sink_len"] = s["n_select"], s["sink"]
            t["tail_start"], t["tail_len"] = s["tail_start"], s["tail_len"]
            t["score_mode"], t["pool_kernel"] = s["score_mode"], s["pool"]
        self.new_outputs()
        rc, self.info = N.plan(self.p, self.table)
        assert rc == 0, rc
        self.ws = None

    def new_outputs(self):
        tdt = self.layers[0][0].dtype
        es = self.layers[0][0].element_size()
        sent = _signed(PT.SENTINEL[self.dtype], 8 * es)
        self.outs = []
        for t, s in zip(self.table, self.specs):
            shape = (self.B, self.H, PT.n_out(s), D)
            ko, vo = (torch.full(shape, sent, dtype=INT[es], device="cuda:0").view(tdt)
                      for _ in range(2))
            t["k_out"], t["v_out"] = ko.data_ptr(), vo.data_ptr()
            self.outs.append((ko, vo))

    def new_workspace(self):
        self.ws = torch.full((int(self.info.workspace_bytes),), PT.POISON, dtype=torch.uint8,
                             device="cuda:0")
        return self.ws

    def launch(self, phases, flags=None):
        self.p.phases = phases
        if flags is not None:
            self.p.flags = flags
        rc = N.launch(self.p, self.table, self.ws.data_ptr(), int(self.info.workspace_bytes),
                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (rc, phases)

    def run(self, phase_list, flags):
        """Fresh outputs and workspace, the launches in order; returns the outputs as bits."""
        self.new_outputs()
        self.new_workspace()
        for ph in phase_list:
            self.launch(ph, flags)
        torch.cuda.synchronize()
        return [(_bits(ko), _bits(vo)) for ko, vo in self.outs]

    def region(self, offset, stride, dtype):
        """[rows, stride] view of a workspace region."""
        rows = int(self.info.rows)
        n = rows * int(stride) * torch.empty(0, dtype=dtype).element_size()
        return self.ws[int(offset):int(offset) + n].view(dtype).view(rows, int(stride))

    def index_rows(self):
        return self.region(self.info.index_offset, self.info.index_row_stride, torch.int32)

    def norm_rows(self):
        return self.region(self.info.norm_offset, self.info.norm_row_stride,
                           INT[self.layers[0][0].element_size()])


_INPUTS = {}


def _inputs(key, specs, B, H, dtype):
    """Host and device K / V of a table, generated once for the run of cases that share them."""
    if key not in _INPUTS:
        _INPUTS.clear()
        host = PT.gen_layers(specs, B, H, D, dtype)
        _INPUTS[key] = (host, [(to_dev(k), to_dev(v)) for k, v in host])
    return _INPUTS[key]


def _as_bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _check_shapes(specs, host, dev, dtype, B, H, order, algo, shapes, index_shapes):
    want = [PT.expected_layer(k, v, s, order, algo) for (k, v), s in zip(host, specs)]
    sent = PT.SENTINEL[dtype]
    for wk, wv, _ in want:
        assert not (_as_bits(wk) == sent).any() and not (_as_bits(wv) == sent).any()
    call = Call(specs, dev, dtype, B, H, order, algo)
    for name in shapes:
        phase_list, flags = SHAPES[name]
        got = call.run(phase_list, flags)
        for li, ((gk, gv), (wk, wv, widx)) in enumerate(zip(got, want)):
            assert not (gk == sent).any() and not (gv == sent).any(), (name, li, "sentinel left")
            assert np.array_equal(gk, _as_bits(wk)), (name, li, "K")
            assert np.array_equal(gv, _as_bits(wv)), (name, li, "V")
        if name in index_shapes:
            idx = call.index_rows().cpu().numpy()
            for t, s, (_, _, widx) in zip(call.table, specs, want):
                k = s["n_select"]
                rows = idx[t["row0"]:t["row0"] + B * H, :k]
                assert np.array_equal(rows, widx.reshape(B * H, k)), (name, "index rows")
        assert int(call.status.item()) == 0, name


# ------------------------------------------------------------------------------------------
# 1. phase splits equal one launch
# ------------------------------------------------------------------------------------------
def _id(c):
    names = {(0, 0): "asc-sort", (1, 0): "desc-sort", (1, 1): "desc-topk", (0, 2): "asc-stable",
             (1, 2): "desc-stable"}
    return f"{c[0]}-{c[1]}-{names[c[2:]]}"


@pytest.mark.parametrize("case", PT.split_cases(), ids=_id)
def test_phase_splits_equal_one_launch(case):
    """PHASE_ALL | SCORE, SELECT|GATHER | SCORE, SELECT, GATHER | PHASE_ALL with the split flag,
    each on its own 0xFF workspace over sentinel outputs: K and V byte-equal to the CPU
    expectation (hence to each other), no sentinel left, the index rows of the two shapes with a
    separate SELECT equal to the oracle's ascending indices, status 0."""
    Z, dtype, order, algo = case
    B, H = PT.split_geometry(Z)
    specs = PT.split_table(Z)
    host, dev = _inputs(("split", Z, dtype), specs, B, H, dtype)
    _check_shapes(specs, host, dev, dtype, B, H, order, algo, list(SHAPES),
                  ("score|select|gather", "all, split flag"))


@pytest.mark.parametrize("case", PT.snapkv_cases(), ids=lambda c: f"{c[0]}-{c[1]}-pool{c[2]}")
def test_snapkv_phase_splits_equal_one_launch(case):
    """KVC_SCORE_SNAPKV rows (DESC + TOPK): SELECT reads the per-tile maxima SCORE left in the
    workspace, so SCORE then SELECT|GATHER -- bench.py --full's split timer -- must equal one
    launch, from a workspace that held 0xFF where those maxima go."""
    Z, dtype, pool = case
    B, H = PT.split_geometry(Z)
    specs = PT.split_table(Z, PT.SNAPKV, pool)
    host, dev = _inputs(("snapkv", Z, dtype), specs, B, H, dtype)
    _check_shapes(specs, host, dev, dtype, B, H, PT.DESC, PT.TOPK,
                  ("all", "score|select+gather", "all, split flag"), ("all, split flag",))


# ------------------------------------------------------------------------------------------
# 2. chunk boundaries under phase splits
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_layers", [65, 129])
def test_chunk_boundary_under_phase_splits(n_layers):
    """More layers than one kernel-argument chunk (64): the per-chunk tile_base / tile_end, row0
    and index rows with the phases launched one by one, every layer against the CPU."""
    specs = PT.chunk_table(n_layers)
    host, dev = _inputs(("chunk", n_layers), specs, 1, 1, "bf16")
    _check_shapes(specs, host, dev, "bf16", 1, 1, PT.ASC, PT.SORT,
                  ("all", "score|select|gather"), ("score|select|gather",))


# ------------------------------------------------------------------------------------------
# 3. SELECT from a norm region the caller wrote
# ------------------------------------------------------------------------------------------
def _norm_groups():
    groups = {}
    for n, dt, pair, k, o, a in PT.norm_cases():
        groups.setdefault((n, dt), []).append((pair, k, o, a))
    return groups


_NORM_GROUPS = _norm_groups()


@pytest.mark.parametrize("n, dtype", list(_NORM_GROUPS), ids=lambda x: str(x))
def test_select_from_caller_written_norms(n, dtype):
    """phases = SELECT, and SELECT|GATHER, on a 0xFF workspace whose norm rows [row, :zone_len]
    the test wrote (values a norm can be: finite, +inf, NaN, sub-normal, 8-valued, all equal):
    with the columns behind zone_len left as poison, zeroed, or set to +inf, the selected set is
    the oracle's for the written values every time.  K and V rows carry their position, so the
    fused SELECT|GATHER kernel's set is read from its output."""
    H = 2
    s = PT.spec(n, zone_start=0, zone_len=n, n_select=1)
    pos = to_dev(PT.prng.encode_positions((1, H, n, D), dtype))
    posf = pos.float()
    for pair in sorted({c[0] for c in _NORM_GROUPS[(n, dtype)]}):
        vals = PT.norm_rows(n, dtype, pair)
        dvals = to_dev(vals).view(INT[pos.element_size()]).view(H, n)
        for p_, k, order, algo in _NORM_GROUPS[(n, dtype)]:
            if p_ != pair:
                continue
            want = np.sort(PT.select(vals, k, order, algo), axis=-1).reshape(H, k)
            dwant = torch.from_numpy(want).to("cuda:0")
            call = Call([dict(s, n_select=k)], [(pos, pos)], dtype, 1, H, order, algo)
            for phases in (SELECT, SELECT | GATHER):
                for pad in PT.PADS:
                    call.new_outputs()
                    call.new_workspace()
                    nr = call.norm_rows()
                    nr[:, :n] = dvals
                    if pad != "poison":
                        padv = to_dev(np.array([PT.pad_value(pad, dtype)]))
                        nr[:, n:] = padv.view(nr.dtype)
                    call.launch(phases, 0)
                    what = (pair, k, order, algo, phases, pad)
                    if phases == SELECT or n > 16384:  # a separate SELECT writes the index rows
                        assert torch.equal(call.index_rows()[:, :k].long(), dwant), what
                    if phases & GATHER:
                        for o in call.outs[0]:
                            got = o[0, :, :, 0].float() * 256 + o[0, :, :, 1].float()
                            assert torch.equal(got.long(), dwant), what
                            assert torch.equal(o[0].float(), posf[0].gather(
                                1, dwant[:, :, None].expand(H, k, D))), what
                    assert int(call.status.item()) == 0, what
