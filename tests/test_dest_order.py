"""The ordering argument of in-place compaction (gather_passes, csrc/kvc_gather_dest.h: the one
pass schedule of the dense and the paged copy kernel), in numpy, no engine.

For every in-place case of tests/dest_cases.py the row map src(t) of each changed layer is read
off the oracle's position-tagged V output.  (a) Copying the output rows onto the input in
DESCENDING order -- a legal schedule of an unordered parallel copy -- gives another result for
every compressed layer: the shapes have read-after-write hazards a naive kernel can hit.  (b) The
kernel's schedule -- ascending passes of P consecutive output rows, all loads of a pass before its
stores -- gives the oracle's rows for every pass size and leaves rows [n_out, S) untouched.
"""
import numpy as np
import pytest

import dest_cases as DC

PASS_ROWS = (1, 7, 64, 512, 4096)


def _changed_layers(case):
    """[(layer index, S, kind, src [B,H,n])] of the layers the call changes."""
    layers, ref = DC.reference(case)
    out = []
    for li, ((k, v), (rk, rv, kind)) in enumerate(zip(layers, ref)):
        if kind == "same":
            continue
        src = DC.row_map(case, rv)
        assert src.shape[2] == rk.shape[2] <= k.shape[2]
        out.append((li, k.shape[2], kind, src))
    return out


def _ids(src, S):
    return np.broadcast_to(np.arange(S, dtype=np.int64), src.shape[:2] + (S,)).copy()


@pytest.mark.parametrize("case", DC.INPLACE, ids=[c["id"] for c in DC.INPLACE])
def test_row_maps_are_strictly_increasing_and_never_point_down(case):
    """What kvc_plan_dest's segment-order rule promises the kernel: src(t) >= t, ascending."""
    changed = _changed_layers(case)
    assert changed
    for li, S, kind, src in changed:
        n = src.shape[2]
        assert (np.diff(src, axis=2) > 0).all(), (case["id"], li)
        assert (src >= np.arange(n)).all() and (src < S).all(), (case["id"], li)


@pytest.mark.parametrize("case", DC.INPLACE, ids=[c["id"] for c in DC.INPLACE])
def test_descending_copy_in_place_corrupts_every_compressed_layer(case):
    """(a) Results that are slices far behind the front (recent_only: sources at S - 512 and up,
    destinations below 512) have no hazard and are left out; every gathered layer has one."""
    compressed = [c for c in _changed_layers(case) if c[2] == "new"]
    for li, S, kind, src in compressed:
        ids, n = _ids(src, S), src.shape[2]
        for t in range(n - 1, -1, -1):
            ids[:, :, t] = np.take_along_axis(ids, src[:, :, t:t + 1], axis=2)[:, :, 0]
        assert not np.array_equal(ids[:, :, :n], src), (case["id"], li)


@pytest.mark.parametrize("rows", PASS_ROWS)
@pytest.mark.parametrize("case", DC.INPLACE, ids=[c["id"] for c in DC.INPLACE])
def test_ascending_passes_with_loads_before_stores_are_a_correct_memmove(case, rows):
    """(b)"""
    for li, S, kind, src in _changed_layers(case):
        ids, n = _ids(src, S), src.shape[2]
        for t0 in range(0, n, rows):
            t1 = min(n, t0 + rows)
            loaded = np.take_along_axis(ids, src[:, :, t0:t1], axis=2)  # every load of the pass
            ids[:, :, t0:t1] = loaded                                   # then its stores
        assert np.array_equal(ids[:, :, :n], src), (case["id"], li, rows)
        assert np.array_equal(ids[:, :, n:], _ids(src, S)[:, :, n:]), (case["id"], li, rows)
