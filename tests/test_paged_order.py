"""The ordering argument of in-place compaction through a block table (the schedule is
gather_passes, csrc/kvc_gather_dest.h; the table's address arithmetic and why distinct logical
rows are distinct bytes, csrc/kvc_paged.h), in numpy, no engine.

A pool [N, H, P] of unique ids stands for K (or V); every batch row owns ceil(S / P) pages of a
seeded permutation and 7 pages stay spare.  For every in-place case of tests/dest_cases.py the row
map src(t) of each changed layer is read off the oracle's position-tagged V output.  (a) The
kernel's schedule -- ascending passes of consecutive output rows, all loads of a pass before its
stores, every row addressed as (table[b, s >> log2 P], s & (P - 1)) -- leaves exactly the pool the
oracle's rows written through the table give, for every pass size: the result, rows [n, S) and the
spare pages in one comparison.  (b) The same schedule with the table ignored, with half or double
the page size, or with batch row 0's table used for row 1 leaves a different pool on the same
inputs -- so the GPU cases (tests/test_paged_gpu.py, same tables) cannot pass with the table wrong.
"""
import numpy as np
import pytest

import dest_cases as DC

P = 16
SPARE = 7
PASS_ROWS = (1, 7, 64, 4096)


def _changed_layers(case):
    layers, ref = DC.reference(case)
    out = []
    for li, ((k, v), (rk, rv, kind)) in enumerate(zip(layers, ref)):
        if kind != "same":
            out.append((li, k.shape[2], DC.row_map(case, rv)))
    return out


def _table(Bn, S, seed):
    npp = -(-S // P)
    perm = np.random.default_rng(seed).permutation(Bn * npp + SPARE)
    return perm[:Bn * npp].reshape(Bn, npp).astype(np.int64), Bn * npp + SPARE


def _addr(tab, Hn, page_size, table_row=None):
    """(b, h, s) -> flat index into a pool [N, H, P]: the kernel's address arithmetic with the
    given page size and table row choice (index and address clamped into their arrays, as a wrong
    kernel's would merely be wrong, not out of the model)."""
    flat = tab.reshape(-1)
    lg = page_size.bit_length() - 1
    stride = tab.shape[1]

    def f(b, h, s, size):
        row = b if table_row is None else table_row(b)
        page = flat[np.minimum(row * stride + (s >> lg), flat.size - 1)]
        return np.minimum(page * Hn * P + h * P + (s & (page_size - 1)), size - 1)
    return f


def _identity_addr(tab, Hn):
    stride = tab.shape[1]

    def f(b, h, s, size):  # the table ignored: sequence b's pages taken as consecutive
        return (b * stride + (s >> 4)) * Hn * P + h * P + (s & (P - 1))
    return f


def _run(addr, src, S, npages, rows):
    """The pass schedule on a pool of unique ids; returns (pool before, pool after)."""
    Bn, Hn, n = src.shape
    pool = np.arange(npages * Hn * P, dtype=np.int64)
    before = pool.copy()
    b = np.arange(Bn)[:, None, None]
    h = np.arange(Hn)[None, :, None]
    for t0 in range(0, n, rows):
        t = np.arange(t0, min(n, t0 + rows))[None, None, :]
        loaded = pool[addr(b, h, src[:, :, t0:t0 + t.shape[2]], pool.size)]  # every load
        pool[np.broadcast_to(addr(b, h, t, pool.size), loaded.shape)] = loaded  # then the stores
    return before, pool


def _expected(tab, src, before, Hn):
    addr = _addr(tab, Hn, P)
    Bn, _, n = src.shape
    b = np.arange(Bn)[:, None, None]
    h = np.arange(Hn)[None, :, None]
    want = before.copy()
    t = np.arange(n)[None, None, :]
    want[np.broadcast_to(addr(b, h, t, want.size), src.shape)] = before[addr(b, h, src, want.size)]
    return want


@pytest.mark.parametrize("rows", PASS_ROWS)
@pytest.mark.parametrize("case", DC.INPLACE, ids=[c["id"] for c in DC.INPLACE])
def test_pass_schedule_through_a_shuffled_table_is_a_correct_memmove(case, rows):
    changed = _changed_layers(case)
    assert changed
    for li, S, src in changed:
        Bn, Hn, n = src.shape
        tab, npages = _table(Bn, S, case["seed"] + li)
        assert len(set(tab.reshape(-1))) == tab.size  # every batch row its own distinct pages
        before, after = _run(_addr(tab, Hn, P), src, S, npages, rows)
        assert np.array_equal(after, _expected(tab, src, before, Hn)), (case["id"], li, rows)


@pytest.mark.parametrize("case", DC.INPLACE, ids=[c["id"] for c in DC.INPLACE])
def test_a_wrong_table_reading_gives_other_bytes(case):
    for li, S, src in _changed_layers(case):
        Bn, Hn, n = src.shape
        tab, npages = _table(Bn, S, case["seed"] + li)
        assert not np.array_equal(tab.reshape(-1), np.arange(tab.size))  # shuffled indeed
        before = np.arange(npages * Hn * P, dtype=np.int64)
        want = _expected(tab, src, before, Hn)
        wrong = {"table ignored": _identity_addr(tab, Hn),
                 "half the page size": _addr(tab, Hn, P // 2),
                 "double the page size": _addr(tab, Hn, P * 2)}
        if Bn > 1:
            wrong["row 0's table for row 1"] = _addr(tab, Hn, P, lambda b: b * 0)
        for name, addr in wrong.items():
            _, after = _run(addr, src, S, npages, 64)
            assert not np.array_equal(after, want), (case["id"], li, name)
