"""Ragged paged batches on the host (include/kvc.h, "Ragged paged batches"): kvc_plan_ragged's
contract through ctypes, the argument checks of PagedKV / compress_paged that need no GPU, the
register / scratch budgets of the new kernels, and a numpy model of the record mapping showing
that the GPU cases (tests/test_ragged_gpu.py) cannot pass with the records ignored.  CPU only."""
import ctypes
import re

import numpy as np
import pytest
import torch

import ragged_util as RU
import test_abi
import test_paged_plan as PP
from kvcompress import _native as N
from test_kernel_budget import _kernels

E_ARG = -1
SEQS = 1 << 22  # a 16-byte aligned "device" address (kvc_plan_ragged dereferences host only)


def _seq(seq_len, sink=0, zs=0, zl=0, k=0, ts=0, tl=0, mode=0, pool=0, n_out=None):
    q = np.zeros(1, dtype=N.SEQ_DTYPE)[0]
    q["seq_len"], q["sink_len"], q["zone_start"], q["zone_len"], q["n_select"] = seq_len, sink, zs, zl, k
    q["tail_start"], q["tail_len"], q["score_mode"], q["pool_kernel"] = ts, tl, mode, pool
    q["n_out"] = sink + k + tl if n_out is None else n_out
    return q


def _noop(seq_len):
    return _seq(seq_len, sink=seq_len)


GOOD = [_seq(1000, 4, 4, 700, 100, 704, 296), _seq(600, 4, 4, 300, 299, 304, 296)]


def _plan(seqs, layer=None, pages=None, host=True, dev=SEQS, launch=False, **pkw):
    seqs = np.array(seqs, dtype=N.SEQ_DTYPE)
    table = np.array([PP._layer(True) if layer is None else layer], dtype=N.LAYER_DTYPE)
    pg = np.array([PP._pages(True) if pages is None else pages], dtype=N.PAGES_DTYPE)
    rg = np.zeros(1, dtype=N.RAGGED_DTYPE)
    rg[0] = (seqs.ctypes.data if host else 0, dev)
    p = PP._params(**pkw)
    rc, info = N.plan_ragged(p, table, pg, rg)
    if launch and rc == 0:  # the launch re-validates before it touches the (absent) workspace
        return N.launch_ragged(p, table, pg, rg, None, 0, None), info, table
    return rc, info, table


def test_struct_sizes_and_declarations():
    assert N.SEQ_DTYPE.itemsize == 48 and N.SEQ_DTYPE.itemsize % 16 == 0
    assert N.RAGGED_DTYPE.itemsize == 16
    assert {"kvc_plan_ragged", "kvc_launch_ragged"} <= set(N.EXPORTS)
    assert {"kvc_plan_ragged", "kvc_launch_ragged"} <= set(test_abi._declared_functions())
    assert N.lib().kvc_version() == 4 and N.lib().kvc_layer_struct_size() == 136


def test_envelope_equals_kvc_plan_of_the_envelope_layer():
    """Two ragged layers (the second with a snapkv record and a no-op one): the segment fields are
    the documented envelope, and every planned field and kvc_plan_info_t are kvc_plan's for it."""
    a = np.array(GOOD, dtype=N.SEQ_DTYPE)
    b = np.array([_noop(37), _seq(900, 0, 0, 868, 480, 868, 32, mode=1, pool=5)],
                 dtype=N.SEQ_DTYPE)
    table = np.array([PP._layer(True), PP._layer(True)], dtype=N.LAYER_DTYPE)
    pages = np.array([PP._pages(True), PP._pages(True)], dtype=N.PAGES_DTYPE)
    rg = np.zeros(2, dtype=N.RAGGED_DTYPE)
    rg[0], rg[1] = (a.ctypes.data, SEQS), (b.ctypes.data, SEQS + 96)
    rc, info = N.plan_ragged(PP._params(), table, pages, rg)
    assert rc == 0
    env = np.array([PP._layer(True, sink=0, zs=0, zl=700, k=299, ts=0, tl=599 - 299, seq_len=1000),
                    PP._layer(True, sink=0, zs=0, zl=868, k=480, ts=0, tl=512 - 480, seq_len=900,
                              score_mode=1, pool_kernel=5)], dtype=N.LAYER_DTYPE)
    rc2, info2 = N.plan(PP._params(), env)
    assert rc2 == 0 and PP._info(info) == PP._info(info2)
    assert table.tobytes() == env.tobytes()
    assert table["n_out"].tolist() == [599, 512]
    # the launch accepts exactly this table (it stops at the workspace), not one with stale fields
    p = PP._params()
    assert N.launch_ragged(p, table, pages, rg, None, 0, None) == -6  # KVC_E_WORKSPACE
    stale = table.copy()
    stale[0]["zone_len"] = 699
    assert N.launch_ragged(p, stale, pages, rg, None, 0, None) == E_ARG


def test_envelope_of_a_selecting_record_selects():
    """One record keeps the longest zone whole while another selects: max n_select == max zone_len,
    and the envelope's zone grows by one so that the layer is still scored and selected."""
    rc, info, table = _plan([_seq(800, 0, 0, 500, 500, 500, 300), _seq(700, 0, 0, 400, 100, 400, 300)])
    assert rc == 0 and int(table[0]["zone_len"]) == 501 and int(table[0]["n_select"]) == 500
    assert info.score_tiles == PP.B * PP.H * 8 and info.norm_row_stride == 512


REJECTED = {
    "zone past seq_len": [GOOD[0], _seq(600, 4, 4, 597, 100, 304, 296)],
    "n_select > zone_len": [GOOD[0], _seq(600, 4, 4, 300, 301, 304, 296)],
    "tail past seq_len": [GOOD[0], _seq(600, 4, 4, 300, 100, 304, 297)],
    "n_out is not the sum": [GOOD[0], _seq(600, 4, 4, 300, 100, 304, 296, n_out=401)],
    "row map: sink behind the zone start": [GOOD[0], _seq(600, 8, 4, 300, 100, 304, 296)],
    "row map: zone into the tail": [GOOD[0], _seq(600, 4, 4, 301, 100, 304, 296)],
    "bad score mode": [GOOD[0], _seq(600, 4, 4, 300, 100, 304, 296, mode=2)],
}


@pytest.mark.parametrize("why", list(REJECTED))
def test_bad_records_are_refused(why):
    assert _plan(GOOD)[0] == 0
    assert _plan(REJECTED[why])[0] == E_ARG, why


def test_table_stride_covers_the_longest_sequence():
    seqs = [_noop(40), GOOD[0]]  # 1000 rows of 16: 63 pages
    assert _plan(seqs, pages=PP._pages(True, table_stride=63))[0] == 0
    assert _plan(seqs, pages=PP._pages(True, table_stride=62))[0] == E_ARG


def test_ragged_layers_are_paged_and_in_place():
    assert _plan(GOOD, pages=PP._pages(False))[0] == E_ARG                 # in_place == 0
    assert _plan(GOOD, layer=PP._layer(False))[0] == E_ARG                 # a dense destination
    assert _plan(GOOD, external_index=1, phases=N.PHASE_GATHER)[0] == E_ARG
    for flag in (N.FLAG_GATHER_FIXED, N.FLAG_GATHER_SELECTED, N.FLAG_SHARED_INDEX):
        assert _plan(GOOD, flags=flag)[0] == E_ARG


def test_null_and_misaligned_record_pointers():
    assert _plan(GOOD, host=False)[0] == E_ARG
    assert _plan(GOOD, dev=0)[0] == E_ARG
    assert _plan(GOOD, dev=SEQS + 4)[0] == E_ARG


def test_noop_records_are_accepted():
    rc, info, table = _plan([_noop(1000), _noop(0)])
    assert rc == 0 and info.score_tiles == 0
    assert int(table[0]["n_out"]) == 1000 and int(table[0]["n_select"]) == 0
    rc, info, table = _plan([_noop(5), GOOD[0]], launch=True)
    assert rc == -6  # valid up to the workspace


def test_null_ragged_table_is_kvc_plan_paged():
    t0 = np.array([PP._layer(True), PP._layer(True, zl=600, k=600, ts=700, tl=300)],
                  dtype=N.LAYER_DTYPE)
    t1 = t0.copy()
    pages = np.array([PP._pages(True)] * 2, dtype=N.PAGES_DTYPE)
    rc0, i0 = N.plan_paged(PP._params(), t0, pages, None)
    rc1, i1 = N.plan_ragged(PP._params(), t1, pages, None)
    assert rc0 == rc1 == 0 and PP._info(i0) == PP._info(i1) and t0.tobytes() == t1.tobytes()
    pages[1]["page_size"] = 3
    assert N.plan_paged(PP._params(), t0, pages, None)[0] == E_ARG
    assert N.plan_ragged(PP._params(), t1, pages, None)[0] == E_ARG


# ---- PagedKV / compress_paged argument checks that run before any device is needed ------------
def _pools(B=3, cols=4):
    k = torch.zeros(8, 2, 16, 64, dtype=torch.bfloat16)
    return k, torch.zeros_like(k), torch.zeros(B, cols, dtype=torch.int32)


def test_paged_kv_length_arguments():
    from kvcompress import PagedKV
    k, v, bt = _pools()
    with pytest.raises(ValueError, match="2 sequence lengths for a block table of 3 rows"):
        PagedKV(k, v, bt, [10, 20])
    with pytest.raises(ValueError, match="non-negative ints, got -1"):
        PagedKV(k, v, bt, [10, -1, 5])
    with pytest.raises(ValueError, match="non-negative ints, got True"):
        PagedKV(k, v, bt, [10, True, 5])
    with pytest.raises(ValueError):
        PagedKV(k, v, bt, True)
    with pytest.raises(ValueError):
        PagedKV(k, v, bt, np.array([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="fewer than the 5 pages of 70 rows"):
        PagedKV(k, v, bt, (10, 70, 5))  # the table's width against the LONGEST sequence
    with pytest.raises(TypeError, match="host data"):
        PagedKV(k, v, bt, torch.zeros(3, dtype=torch.int64, device="meta"))
    # every accepted spelling gets as far as the device check, which names no length
    for lens in ([10, 64, 0], (10, 64, 0), np.array([10, 64, 0], dtype=np.int32),
                 torch.tensor([10, 64, 0]), 64):
        with pytest.raises(ValueError, match="must be on one ROCm device"):
            PagedKV(k, v, bt, lens)


def test_plan_ragged_maps_methods_onto_records():
    """The host planning alone (no GPU): one method run per distinct profile, records and new
    lengths per (layer, sequence), layer indices kept (the skip list)."""
    from kvcompress import paged
    from kvcompress.methods import get_compress_fn
    lens = [[0, 37, 512, 513, 1500, 513]] * 2
    geo = [(2, 64, torch.bfloat16, torch.device("cpu"))] * 2
    rec, how, new = paged.plan_ragged(get_compress_fn("fix_size_l2"), lens, geo,
                                      dict(fix_kv_size=512, keep_ratio=0.25, skip_layers=[0]),
                                      check=False)
    assert new == [[0, 37, 512, 513, 1500, 513], [0, 37, 512, 512, 512, 512]]
    assert set(how) == {(1, 3), (1, 4), (1, 5)}
    assert all(h == (N.KVC_ASC, N.KVC_ALGO_SORT) for h in how.values())
    r = rec[1, 3]  # the decode-shaped row: k = n - 1
    assert (int(r["zone_len"]), int(r["n_select"]), int(r["tail_len"])) == (385, 384, 128)
    assert rec[1, 3].tobytes() == rec[1, 5].tobytes()
    for li, b in ((0, 4), (1, 0), (1, 2)):  # skipped layer / passed-through sequences: no-op
        q = rec[li, b]
        assert int(q["sink_len"]) == int(q["n_out"]) == int(q["seq_len"]) == lens[li][b]
        assert int(q["n_select"]) == int(q["tail_len"]) == int(q["zone_len"]) == 0


# ---- budgets ------------------------------------------------------------------------------------
def test_ragged_stream_kernels_do_not_spill(tmp_path):
    """Every score_ragged_kernel (rows up to 512 bytes, the bound of the paged budget test) and
    every gather_ragged_kernel instance: no private segment, no spills."""
    ks = _kernels(tmp_path)
    score = {n: v for n, v in ks.items()
             if re.match(r"_ZN3kvc19score_ragged_kernelILi\dELi(4|8|10|16|20|32)E", n)}
    gather = {n: v for n, v in ks.items() if re.match(r"_ZN3kvc20gather_ragged_kernelILi\dELi\d+E", n)}
    assert len(score) == 18 and len(gather) == 21, (sorted(score), sorted(gather))
    for n, v in {**score, **gather}.items():
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)


def test_ragged_select_kernels_fit_two_rows_per_cu(tmp_path):
    """The 16-bit-key ragged SELECT instances meet test_select_kernels_fit_two_rows_per_cu's
    bound: at most 64 VGPRs, no scratch."""
    ks = _kernels(tmp_path)
    hot = {n: v for n, v in ks.items()
           if re.match(r"_ZN3kvc20select_ragged_kernelILi1ELi(512|1024)ELb0E", n)}
    assert len(hot) == 2, sorted(ks)
    for n, v in hot.items():
        assert v["vgpr_count"] <= 64, (n, v)
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)


# ---- power: the GPU cases cannot pass with the records ignored ----------------------------------
def _model(seqs, records):
    """numpy model of one fix_size_l2-style layer (plain norms, ascending sort) under `records`
    (one per sequence): sink ++ zone[selected] ++ tail, bounds clipped to the sequence as a kernel
    reading a wrong record would find them clamped or poisoned.  Returns [(K_out, V_out)]."""
    from oracle import oracle
    out = []
    for (k, v), q in zip(seqs, records):
        S = k.shape[2]
        sink, zs, zl, ns = (int(q[f]) for f in ("sink_len", "zone_start", "zone_len", "n_select"))
        ts, tl = int(q["tail_start"]), int(q["tail_len"])
        if ns == 0 and tl == 0:  # a no-op record
            out.append((k[:, :, :min(sink, S)], v[:, :, :min(sink, S)]))
            continue
        zk, zv = k[:, :, zs:min(zs + zl, S)], v[:, :, zs:min(zs + zl, S)]
        kk, kv = zk[:, :, :0], zv[:, :, :0]
        if 0 < ns and zk.shape[2] > 0:
            idx = oracle.select_low(zk, min(ns, zk.shape[2]))
            kk, kv = oracle.gather(zk, idx), oracle.gather(zv, idx)
        out.append((oracle.cat([k[:, :, :min(sink, S)], kk, k[:, :, ts:min(ts + tl, S)]]),
                    oracle.cat([v[:, :, :min(sink, S)], kv, v[:, :, ts:min(ts + tl, S)]])))
    return out


def test_gpu_cases_fail_with_the_records_ignored():
    """The model with every sequence's OWN record reproduces the per-sequence oracle on the
    every-method lengths; with sequence 0's record for all, or with the envelope for all, it does
    not -- for every sequence that compresses, and for a passed-through one under the envelope."""
    from kvcompress import paged
    from kvcompress.methods import get_compress_fn
    kw = dict(fix_kv_size=512, keep_ratio=0.25, skip_layers=[])
    lens, Hh, D = RU.LENS, RU.H, 64
    seqs = RU.gen_sequences(977, lens, Hh, D, "bf16")
    ref = RU.oracle_per_sequence("fix_size_l2", kw, [seqs])[0]
    rec, _, new = paged.plan_ragged(get_compress_fn("fix_size_l2"), [lens],
                                    [(Hh, D, torch.bfloat16, torch.device("cpu"))], kw,
                                    check=False)
    assert new[0] == [r[0].shape[2] for r in ref] == [0, 37, 512, 512, 512]

    def same(got, b):
        return all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got[b], ref[b][:2]))

    own = _model(seqs, rec[0])
    assert all(same(own, b) for b in range(len(lens)))
    seq0 = _model(seqs, [rec[0, 0]] * len(lens))         # sequence 0 is empty: everything "passes"
    assert not same(seq0, 3) and not same(seq0, 4)
    env = np.zeros(1, dtype=N.SEQ_DTYPE)[0]
    env["seq_len"], env["zone_len"] = max(lens), int(rec[0]["zone_len"].max())
    env["n_select"] = int(rec[0]["n_select"].max())
    env["tail_len"] = int(rec[0]["n_out"].max()) - int(env["n_select"])
    env["n_out"] = int(rec[0]["n_out"].max())
    under_env = _model(seqs, [env] * len(lens))
    assert not any(same(under_env, b) for b in (1, 2, 3, 4))


# ---- the sweep's generator covers what the GPU sweep is meant to ----------------------------------
def test_sweep_generator_floors():
    from oracle import oracle
    cases = RU.sweep_cases()
    assert len(cases) == 64 and len({c["id"] for c in cases}) == 64
    assert {c["method"] for c in cases} == {m for m, _, _ in RU.METHOD_CASES}
    assert all(2 <= len(c["lens"]) <= 6 and 0 <= min(c["lens"]) for c in cases)
    assert sum(max(c["lens"]) > 4096 for c in cases) >= 6
    assert all(max(c["lens"]) <= 2000 for c in cases if max(c["lens"]) <= 4096)
    assert {c["P"] for c in cases} >= {1, 16, 64} and {c["dtype"] for c in cases} == {"bf16", "fp16", "fp32"}
    assert {c["storages"] for c in cases} >= {("nhpd", "nphd"), ("nphd", "nhpd")}
    mixed = 0
    for c in cases:  # shapes alone decide what passes through: one-element rows are enough
        kinds = set()
        for n in c["lens"]:
            kv = (np.zeros((1, 1, n, 8), np.float32), np.zeros((1, 1, n, 8), np.float32))
            out = oracle.METHODS[c["method"]]([kv] * c["L"], **c["kw"])
            kinds |= {(l, o[0].shape[2] == n) for l, o in enumerate(out)}
        mixed += any((l, True) in kinds and (l, False) in kinds for l in range(c["L"]))
    assert mixed >= 32, mixed
