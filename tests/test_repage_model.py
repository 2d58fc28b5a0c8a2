"""A numpy model of the paged-destination delivery (tests/repage_util.py, `deliver`; include/kvc.h,
"Paged destinations") and the proof that the GPU cases of tests/test_repage_gpu.py have teeth.

The model reads the source through the source table and writes rows -- and scale words where
present -- through the destination table at the destination page size.  It is held against
expected buffers built the way the GPU tests build them: the oracle's (or the generator's) output
rows written into a snapshot through the destination table, here by a row-at-a-time loop that
shares no code with the model.  Case 1 is a GPU case itself: dest_cases' h2o_l2 case, its row map
read off the oracle's output, into fresh pages of the same pool and into pages of another size.
The cases named 3, 6 and 7 have the SHAPE of GPU cases 3 (three sequences of 600 rows over one
physical prefix of 512, P = 16), 6 (a ragged call with an empty, a passed-through and compressed
sequences) and 7 (K / V scale-word pools beside the rows, same pools and another pool), but
synthetic rows and seeded row maps of their own, not the GPU tests' generators: what they show is
that a whole-buffer comparison through the destination table, as the GPU tests make it, tells
each of the four wrong engines from the right one on data of that shape -- not that the GPU
cases' own bytes would.  CPU only."""
import numpy as np
import pytest

import dest_cases as DC
import repage_util as RP

WRONG = ("src_table", "src_psize", "scales_stay", "no_passthrough")
POISON = 0x5A5A


def _write_loop(pool, table_row, P, rows):
    """The expectation's writer: one row at a time."""
    for t in range(rows.shape[1]):
        pool[table_row[t // P], :, t % P] = rows[:, t]


def _pool(n_pages, H, P, tail, dtype=np.uint16):
    return np.full((n_pages, H, P) + tail, POISON, dtype=dtype)


def _setup(dense, P_src, new_lens, P_dst, same, seed, scales=False, shared=0):
    """Pools holding dense[b] = (K, V[, ks, vs]) arrays [H, len_b, ...] behind a seeded source
    table (`shared` leading pages common to all sequences), and destination tables/pools."""
    B, H = len(dense), dense[0][0].shape[0]
    lens = [d[0].shape[1] for d in dense]
    own = [-(-n // P_src) - shared for n in lens]
    n_src = shared + sum(own)
    n_dst = RP.pages_for(new_lens, P_dst)
    n_pages = n_src + (n_dst if same else 0) + RP.SPARE
    perm = np.random.default_rng(seed).permutation(n_pages)
    tails = [x.shape[2:] for x in dense[0]]
    pools = [_pool(n_pages, H, P_src, t, x.dtype) for t, x in zip(tails, dense[0])]
    src_tables, at = [], shared
    for b in range(B):
        row = np.concatenate([perm[:shared], perm[at:at + own[b]]])
        at += own[b]
        src_tables.append(row)
        for pool, x in zip(pools, dense[b]):
            _write_loop(pool, row, P_src, x)
    if same:
        dperm, dst_pools = perm[n_src:], pools
    else:
        dperm = np.random.default_rng(seed + 1).permutation(n_dst + RP.SPARE)
        dst_pools = [_pool(n_dst + RP.SPARE, H, P_dst, t, x.dtype) for t, x in zip(tails, dense[0])]
    dst_tables, at = [], 0
    for n in new_lens:
        k = -(-n // P_dst)
        dst_tables.append(dperm[at:at + k])
        at += k
    return pools, src_tables, dst_pools, dst_tables


def _expected(pools, dst_pools, dst_tables, P_dst, dense, maps):
    want = [p.copy() for p in dst_pools]
    for b, m in enumerate(maps):
        if m is None:
            continue
        for w, x in zip(want, dense[b]):
            idx = m.reshape(m.shape + (1,) * (x.ndim - 2))
            _write_loop(w, dst_tables[b], P_dst, np.take_along_axis(x, idx, axis=1))
    return want


def _run(dense, maps, P_src, P_dst, same, seed, wrong=None, shared=0):
    new_lens = [0 if m is None else m.shape[1] for m in maps]
    pools, st, dpools, dt = _setup(dense, P_src, new_lens, P_dst, same, seed, shared=shared)
    want = _expected(pools, dpools, dt, P_dst, dense, maps)
    src_before = [p.copy() for p in pools]
    RP.deliver(pools, st, P_src, dpools, dt, P_dst, maps, wrong=wrong)
    same_bytes = all(np.array_equal(g, w) for g, w in zip(dpools, want))
    if not same and wrong is None:
        assert all(np.array_equal(p, q) for p, q in zip(pools, src_before))
    return same_bytes


# ---- the cases ------------------------------------------------------------------------------
def _method_case():
    """GPU case 1, reduced: dest_cases' h2o_l2 case; the row map is read off the oracle's
    position-tagged V output, the expected K rows are the oracle's K output."""
    case = next(c for c in DC.INPLACE if c["id"] == "h2o_l2-4-64-444-D32")
    layers, ref = DC.reference(case, tagged=True)
    (k, v), (rk, rv, _) = layers[0], ref[0]
    pos = DC.row_map(case, rv)
    dense = [(np.ascontiguousarray(k[b]).view(np.uint16), np.ascontiguousarray(v[b]).view(np.uint16))
             for b in range(k.shape[0])]
    for b in range(k.shape[0]):  # the map reproduces the oracle's rows (gather's NaN rewrite aside)
        assert np.array_equal(np.take_along_axis(dense[b][0], pos[b][..., None], axis=1),
                              np.ascontiguousarray(rk[b]).view(np.uint16))
    return dense, [pos[b] for b in range(k.shape[0])]


def _random_map(rng, H, n, keep):
    if n <= keep:
        return np.broadcast_to(np.arange(n), (H, n)).copy()
    rows = []
    for _ in range(H):
        mid = np.sort(rng.permutation(np.arange(4, n - 32))[:keep - 36])
        rows.append(np.concatenate([np.arange(4), mid, np.arange(n - 32, n)]))
    return np.stack(rows)


def _synthetic(lens, H, D, seed, scales=False, prefix=0):
    rng = np.random.default_rng(seed)
    dense = []
    for n in lens:
        xs = [rng.integers(0, 0x7F00, (H, n, D), dtype=np.uint16) for _ in range(2)]
        if scales:
            xs += [rng.integers(0, 2 ** 32, (H, n), dtype=np.uint32) for _ in range(2)]
        dense.append(tuple(xs))
    for b in range(1, len(lens) if prefix else 0):
        for x, x0 in zip(dense[b], dense[0]):
            x[:, :prefix] = x0[:, :prefix]
    return dense, [(_random_map(rng, H, n, 100) if n else np.zeros((H, 0), dtype=np.int64))
                   for n in lens]


def _cases():
    """name -> (dense, maps, P_src, P_dst, same pool, shared pages)."""
    out = {}
    dense, maps = _method_case()
    out["1 method, same pool"] = (dense, maps, 16, 16, True, 0)
    out["1 method, pages of 4"] = (dense, maps, 16, 4, False, 0)
    dense, maps = _synthetic([600] * 3, 2, 8, 1, prefix=512)
    out["3 shared prefix"] = (dense, maps, 16, 16, True, 512 // 16)
    dense, maps = _synthetic([0, 37, 300, 513], 2, 8, 2)
    maps[0] = None  # an empty sequence: n_out == 0, nothing moves
    out["6 ragged"] = (dense, maps, 16, 16, True, 0)
    dense, maps = _synthetic([300, 37], 2, 8, 3, scales=True)
    out["7 scales"] = (dense, maps, 16, 16, True, 0)
    dense, maps = _synthetic([300], 2, 8, 4, scales=True)
    out["7 scales, other pool"] = (dense, maps, 16, 64, False, 0)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_model_reproduces_the_expected_buffers(name):
    dense, maps, P_src, P_dst, same, shared = CASES[name]
    assert _run(dense, maps, P_src, P_dst, same, 7, shared=shared), name


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_engine_gives_other_bytes(wrong):
    differs = []
    for name, (dense, maps, P_src, P_dst, same, shared) in CASES.items():
        if wrong == "src_table" and not same:
            continue  # (source page ids mean nothing in another pool)
        if not _run(dense, maps, P_src, P_dst, same, 7, wrong=wrong, shared=shared):
            differs.append(name)
    assert differs, wrong
    want = {"src_table": "1 method, same pool", "src_psize": "1 method, pages of 4",
            "scales_stay": "7 scales", "no_passthrough": "6 ragged"}[wrong]
    assert want in differs, (wrong, differs)


def test_the_cases_cover_what_the_wrong_engines_need():
    dense, maps, *_ = CASES["6 ragged"]
    assert maps[0] is None and (maps[1] == np.arange(37)).all() and maps[3].shape[1] == 100
    assert any(len(d) == 4 for d, *_ in CASES.values())            # scale pools
    assert any(ps != pd for _, _, ps, pd, _, _ in CASES.values())  # another page size
