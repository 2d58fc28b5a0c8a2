"""What the delivery-path fuzz (tests/delivery_cases.py, run on the GPU by
tests/test_delivery_fuzz_gpu.py) can tell apart -- shown on the oracle alone, in numpy, no engine.

The oracle runs over every case once (row maps from position-tagged V; delivery_cases.row_maps),
and the survey is held to floors: every path meets every row width (NC) with a layer that really
selects, all three result kinds, copies longer than one pass on the in-place paths, every page
size, every in-place input layout at several lengths, long zones on every path.  Caps keep the
exits of the GPU test rare: calls an in-place plan may refuse, calls the oracle itself refuses.  Then four wrong deliveries are modelled on the
cases' own tables, storages, destinations and row maps, and each must leave other bytes than the
right one.
"""
import numpy as np
import pytest

import delivery_cases as DV

NCS = (4, 8, 10, 16, 20, 32, 64)


class _Survey:
    rows = None


def _survey():
    """One record per case: the case without its arrays, kinds, row maps, lengths."""
    if _Survey.rows is None:
        rows = []
        for case in range(DV.N_CASES):
            c = DV.gen(case, tagged=True)
            # kinds and row maps need the keys alone: one oracle run on position-tagged V; the
            # case's own V only where its gathered bytes are looked at (v_rewrite, below)
            tagged = c["path"] in ("inplace", "paged_inplace")
            own_v = tagged or (any(c["v_patterns"]) and not c["long"])
            ref = DV.reference(c)
            rec = {k: v for k, v in c.items() if k != "layers"}
            rec["S"] = [k.shape[2] for k, _ in c["layers"]]
            rec["BH"] = c["layers"][0][0].shape[:2]
            rec["raised"] = isinstance(ref, Exception)
            if rec["raised"]:
                rec["kinds"], rec["src"] = [], []
            else:
                rec["kinds"] = [kind for _, _, kind in ref]
                rec["src"] = DV.decode_row_maps(ref, c["dtype"])
                for (rk, rv, kind), src in zip(ref, rec["src"]):
                    assert (src is None) == (kind == "same")
                    assert src is None or src.shape[2] == rk.shape[2]
            # a gathered V whose bytes are not its source rows': torch.gather's NaN rewrite shows
            rec["v_rewrite"] = False
            if not rec["raised"] and not tagged and own_v:
                own = [(k, DV.values(c, li, k.shape)) for li, (k, _) in enumerate(c["layers"])]
                for (k, v), (rk, rv, kind), src in zip(own, DV.reference(dict(c, layers=own)),
                                                       rec["src"]):
                    if kind == "new":
                        plain = np.take_along_axis(v, src[..., None], axis=2)
                        rec["v_rewrite"] |= plain.tobytes() != np.ascontiguousarray(rv).tobytes()
            rec["inplace_layers"] = DV.inplace_layers(c)
            rows.append(rec)
        _Survey.rows = rows
    return _Survey.rows


def _on(path):
    return [r for r in _survey() if r["path"] == path and not r["raised"]]


def _selects(r):
    """Layers of kind "new" with a selecting zone."""
    return [li for li, (kind, src) in enumerate(zip(r["kinds"], r["src"]))
            if kind == "new" and DV.selecting(src)]


def _zone(src, S):
    """Length of the zone a row map selects from: S without the leading rows that stay where they
    are and the trailing run that ends at the input's last row (rough where a selection happens
    to keep its zone's first or last rows)."""
    n = src.shape[2]
    tail = (src == S - n + np.arange(n)).all(axis=(0, 1))
    t = int(n if tail.all() else np.argmin(tail[::-1]))
    return S - _sink(src) - t


def _sink(src):
    """Leading output rows that stay where they are in every (b, h)."""
    same = (src == np.arange(src.shape[2])).all(axis=(0, 1))
    return int(src.shape[2] if same.all() else np.argmin(same))


def test_the_generator_is_deterministic_and_stratified():
    a, b = DV.gen(37), DV.gen(37)
    assert a["kw"] == b["kw"] and all(x[0].tobytes() == y[0].tobytes() and
                                      x[1].tobytes() == y[1].tobytes()
                                      for x, y in zip(a["layers"], b["layers"]))
    assert DV.N_CASES <= 320
    rows = _survey()
    for path in DV.PATHS:
        mine = [r for r in rows if r["path"] == path]
        assert {(r["dtype"], r["D"]) for r in mine} == set(DV.WIDTHS), path
        assert {r["method"] for r in mine} == set(DV.METHODS), path
        assert {r["tie"] for r in mine} == {"reference", "stable"}, path
        assert any(r["long"] for r in mine), path
    longs = [r for r in rows if r["long"]]
    assert len(rows) // 12 <= len(longs) <= len(rows) // 8
    assert any(8192 < s <= 16384 for r in longs for s in r["S"])
    assert any(s > 16384 for r in longs for s in r["S"])
    assert {r["BH"][0] for r in rows} == {1, 2} and {r["BH"][1] for r in rows} == {1, 2, 3, 4}
    assert {len(r["S"]) for r in rows} == {1, 2, 3, 4}
    assert {bool(r["kw"]["skip_layers"]) for r in rows} == {False, True}


@pytest.mark.parametrize("path", DV.PATHS)
def test_every_path_meets_every_width_with_a_selecting_layer(path):
    count = {nc: 0 for nc in NCS}
    for r in _on(path):
        count[r["nc"]] += bool(_selects(r))
    assert all(n >= 2 for n in count.values()), (path, count)


@pytest.mark.parametrize("path", DV.PATHS)
def test_every_path_sees_every_kind_and_tiny_results(path):
    mine = _on(path)
    assert {k for r in mine for k in r["kinds"]} == {"same", "view", "new"}, path
    assert any(src is not None and 1 <= src.shape[2] <= 3 for r in mine for src in r["src"]), path
    # ragged lengths and a skipped layer beside compacted ones in one call
    assert any(len(set(r["S"])) > 1 and len(set(r["kinds"])) > 1 for r in mine), path
    assert any(r["kw"]["skip_layers"] and "new" in r["kinds"] for r in mine), path


@pytest.mark.parametrize("path", ["inplace", "paged_inplace"])
def test_in_place_copies_longer_than_one_pass_at_every_width(path):
    count = {nc: 0 for nc in NCS}
    for r in _on(path):
        moved = [src.shape[2] - _sink(src) for src in r["src"] if src is not None]
        count[r["nc"]] += any(m > DV.dest_pass_rows(r["nc"]) for m in moved)
    assert all(n >= 1 for n in count.values()), (path, count)


@pytest.mark.parametrize("path", ["paged_inplace", "paged_dense"])
def test_every_page_size_meets_a_selecting_layer_and_no_table_is_the_identity(path):
    mine = _on(path)
    assert {r["P"] for r in mine if _selects(r)} == set(DV.PAGE_SIZES), path
    assert {(r["k_storage"], r["v_storage"]) for r in mine} == \
        {(a, b) for a in DV.STORAGES for b in DV.STORAGES}, path
    wide = 0
    for r in mine:
        for tab, n_pages, cols in r["tables"]:
            assert len(set(tab.reshape(-1))) == tab.size and tab.max() < n_pages
            assert n_pages == tab.size + DV.SPARE
            wide += cols > tab.shape[1]
            if tab.shape[1] > 1:
                assert any(not (np.diff(row) == 1).all() for row in tab), (r["case"], "identity")
    assert 0 < wide < sum(len(r["tables"]) for r in mine)


def test_every_in_place_input_layout_meets_a_gathered_layer():
    mine = [r for r in _on("inplace") if "new" in r["kinds"]]
    assert {r["k_layout"] for r in mine} == set(DV.INPLACE_LAYOUTS)
    assert {r["v_layout"] for r in mine} == set(DV.INPLACE_LAYOUTS)
    assert any(r["k_layout"] != r["v_layout"] for r in mine)
    strided = _on("strided")
    for lay in DV.COPIED_LAYOUTS:
        assert any(lay in (r["k_layout"], r["v_layout"]) for r in strided), lay
    assert all(r["D"] == 64 and r["dtype"] != "fp32" for r in strided
               if set((r["k_layout"], r["v_layout"])) & set(DV.COPIED_LAYOUTS))
    for path in ("strided", "paged_dense"):
        mixed = [r for r in _on(path) if r["no_pair"] is not None]
        multi = [r for r in _on(path) if len(r["S"]) > 1]
        assert len(multi) // 6 <= len(mixed) <= len(multi) // 2, path
        assert {r["dst_layouts"] for r in _on(path)} == {("static", "bshd"), ("bshd", "static")}
    assert {r["no_pair"][1] for r in _on("strided") if r["no_pair"]} == {None, "inplace"}


def test_every_in_place_layout_meets_several_lengths():
    """K of every layout the engine compacts in place -- the thirds of a fused QKV buffer, where
    K and V share their storage, included -- is gathered at three length strata or more, and its
    copies longer than one pass are not left to the long cases."""
    for lay in DV.INPLACE_LAYOUTS:
        mine = [r for r in _on("inplace") if r["k_layout"] == lay and not r["long"]]
        assert len({r["S0"] for r in mine if "new" in r["kinds"]}) >= 3, lay
        assert any(src.shape[2] - _sink(src) > DV.dest_pass_rows(r["nc"])
                   for r in mine for src in r["src"] if src is not None), lay
    pairs = {(r["k_layout"], r["S0"]) for r in _on("inplace") if not r["long"]}
    assert len(pairs) == len(DV.INPLACE_LAYOUTS) * len(DV.S0S)


@pytest.mark.parametrize("path", DV.PATHS)
def test_long_cases_select_inside_long_zones(path):
    """Under the reference tie policy every path gathers from a zone in (8192, 16384] (the
    1024-thread select in front of its copy kernel) and from one above 16 384 (the global-scratch
    select)."""
    zones = [_zone(src, S) for r in _on(path) if r["long"] and r["tie"] == "reference"
             for src, S, kind in zip(r["src"], r["S"], r["kinds"])
             if kind == "new" and DV.selecting(src)]
    assert any(8192 < z <= 16384 for z in zones), (path, zones)
    assert any(z > 16384 for z in zones), (path, zones)
    changed = [r for r in _on(path) if r["long"] and "new" in r["kinds"]]
    assert len(changed) >= 6, path


def test_refusals_and_oracle_errors_stay_rare():
    rows = _survey()
    assert sum(r["raised"] for r in rows) <= len(rows) // 20
    inplace = [r for r in rows if r["inplace_layers"] and not r["raised"]]
    refusable = [r for r in inplace
                 if any(DV.refusable(r["src"][li], r["S"][li]) for li in r["inplace_layers"])]
    assert len(refusable) <= len(inplace) // 20, [r["case"] for r in refusable]
    # most calls change something: the point of narrowing the kwargs ranges
    changed = [r for r in rows if not r["raised"] and set(r["kinds"]) != {"same"}]
    assert len(changed) >= len(rows) * 3 // 4


@pytest.mark.parametrize("path", ["strided", "paged_dense"])
def test_gathered_values_carry_rewritten_nans(path):
    """V of every third layer holds every NaN pattern of its dtype: a copy without torch.gather's
    rewrite on V (16-bit types) leaves other bytes."""
    mine = [r for r in _on(path) if r["v_rewrite"]]
    assert len(mine) >= 5 and {r["dtype"] for r in mine} == {"bf16", "fp16"}, path


# ---- mutants: wrong deliveries modelled on the cases -------------------------------------------
def _pool_addr(storage, H, P):
    """(page, h, slot) -> element index of a pool backing stored `storage`."""
    if storage == "nhpd":
        return lambda pg, h, sl: (pg * H + h) * P + sl
    return lambda pg, h, sl: (pg * P + sl) * H + h


def _paged_reads(r, li, table_of, k_storage):
    """Ids [B, H, n] the gather of layer li reads from a pool of unique ids that holds logical row
    s of (b, h) at (table[b, s // P], h, s % P) in `r`'s true storage -- looked up through
    `table_of(tab)` and addressed as `k_storage`."""
    tab, n_pages, _ = r["tables"][li]
    (B, H), P, S, src = r["BH"], r["P"], r["S"][li], r["src"][li]
    true = _pool_addr(r["k_storage"], H, P)
    seen = _pool_addr(k_storage, H, P)
    pool = np.full(n_pages * H * P, -1, dtype=np.int64)
    b = np.arange(B)[:, None, None]
    h = np.arange(H)[None, :, None]
    s = np.arange(S)[None, None, :]
    pool[true(tab[b, s // P], h, s % P)] = (b * H + h) * S + s
    use = table_of(tab)
    return pool[seen(use[b, src // P], h, src % P)], (b * H + h) * S + src


@pytest.mark.parametrize("path", ["paged_inplace", "paged_dense"])
def test_mutant_block_table_ignored(path):
    hit = 0
    for r in _on(path):
        for li, src in enumerate(r["src"]):
            if src is not None and src.size:
                ident = lambda tab: np.arange(tab.size).reshape(tab.shape)  # noqa: E731
                got, want = _paged_reads(r, li, ident, r["k_storage"])
                hit += not np.array_equal(got, want)
    assert hit >= 10, path


@pytest.mark.parametrize("path", ["paged_inplace", "paged_dense"])
def test_mutant_pool_storage_orders_swapped(path):
    hit = 0
    for r in _on(path):
        for li, src in enumerate(r["src"]):
            if src is not None and src.size and r["k_storage"] != r["v_storage"]:
                got, want = _paged_reads(r, li, lambda tab: tab, r["v_storage"])
                hit += not np.array_equal(got, want)
    assert hit >= 10, path


@pytest.mark.parametrize("path", ["strided", "paged_dense"])
def test_mutant_destination_strides_taken_as_contiguous(path):
    hit = 0
    for r in _on(path):
        B, H = r["BH"]
        for li, src in enumerate(r["src"]):
            if li in r["inplace_layers"] or (r["no_pair"] and r["no_pair"][0] == li):
                continue
            n = r["S"][li] if src is None else src.shape[2]
            if n == 0:
                continue
            Sd = n + DV.DST_EXTRA
            T = Sd + DV.DST_PAD
            for layout in r["dst_layouts"]:
                start = DV.DST_START[layout]
                back = np.arange(B * H * T, dtype=np.int64).reshape(
                    (B, H, T) if layout == "static" else (B, T, H))
                rows = back if layout == "static" else back.transpose(0, 2, 1)
                win = rows[:, :, start:start + Sd]
                right = np.zeros(back.size, dtype=bool)
                right[win[:, :, :n].reshape(-1)] = True
                off = int(win[0, 0, 0])
                b = np.arange(B)[:, None, None]
                h = np.arange(H)[None, :, None]
                t = np.arange(n)[None, None, :]
                flat = off + (b * H + h) * Sd + t  # the window's rows with contiguous strides
                assert flat.max() < back.size     # a wrong kernel's stores stay inside the cache
                wrong = np.zeros(back.size, dtype=bool)
                wrong[flat.reshape(-1)] = True
                hit += not np.array_equal(right, wrong)
    assert hit >= 10, path


@pytest.mark.parametrize("path", ["inplace", "paged_inplace"])
def test_mutant_in_place_copy_in_one_descending_pass(path):
    hit = 0
    for r in _on(path):
        for li, (src, kind) in enumerate(zip(r["src"], r["kinds"])):
            if src is None or DV.refusable(src, r["S"][li]) or src.shape[2] > 4000:
                continue  # (the long cases are left out: a Python loop over their rows)
            S, n = r["S"][li], src.shape[2]
            ids = np.broadcast_to(np.arange(S, dtype=np.int64), src.shape[:2] + (S,)).copy()
            for t in range(n - 1, -1, -1):
                ids[:, :, t] = np.take_along_axis(ids, src[:, :, t:t + 1], axis=2)[:, :, 0]
            hit += not np.array_equal(ids[:, :, :n], src)
            # ... while the kernel's schedule (ascending passes, loads before stores) is right
            ids = np.broadcast_to(np.arange(S, dtype=np.int64), src.shape[:2] + (S,)).copy()
            rows = DV.dest_pass_rows(r["nc"])
            for t0 in range(0, n, rows):
                t1 = min(n, t0 + rows)
                ids[:, :, t0:t1] = np.take_along_axis(ids, src[:, :, t0:t1], axis=2)
            assert np.array_equal(ids[:, :, :n], src), (r["case"], li)
    assert hit >= 10, path
