"""Paged destinations for the tests (tests/test_repage_*.py): destination block tables and pools,
and the numpy model of the delivery.

GPU side: a Dest is the destination of one tests/paged_util.py Layer (or ragged_util RaggedLayer,
or scaled_gpu ScaledPool): either FRESH PAGES OF THE LAYER'S OWN POOL -- the layer is then built
with room for them (`room`), and they are the next ids of the pool's seeded permutation, so they
are neither source pages nor the 7 spare ones -- or a SEPARATE poisoned pool of any page size and
storage.  Checks compare whole backing buffers, as paged_util does: take a snapshot, write the
expected rows into it through the DESTINATION table, compare every byte.

CPU side (numpy only): `deliver` is the model of include/kvc.h, "Paged destinations"; its `wrong`
argument selects one of four wrong engines (tests/test_repage_model.py).
"""
import numpy as np

SPARE = 7


def pages_for(lens, P):
    return sum(-(-n // P) for n in lens)


# ---------------------------------------------------------------------------------------------
# GPU: destinations
# ---------------------------------------------------------------------------------------------
def room(B, S, P, n_dst):
    """n_pages of a paged_util.Layer that also holds fresh pages for n_dst rows per sequence."""
    return B * -(-S // P) + B * -(-n_dst // P) + SPARE


class Dest:
    """Destination pages of B sequences of up to `n_rows` rows (a list: per sequence).

    same pool (pool = (kb, vb, k, v, k_storage, v_storage) of the source, `used` source pages,
    `seed` the source pool's permutation seed): the page ids after the first `used` of the
    permutation.  Separate pool (pool = None): own poisoned backings [n_pages, ...] of page size
    P in the given storages and a seeded table of its own.  The device table has `extra` more
    columns than needed, holding -1."""

    def __init__(self, n_rows, P, seed, H=None, D=None, dtype=None, pool=None, used=0,
                 storages=("nphd", "nhpd"), extra=1):
        import torch
        import paged_util as PU
        npp = [-(-n // P) for n in n_rows]
        B = len(n_rows)
        self.P, self.same = P, pool is not None
        if pool is not None:
            self.kb, self.vb, self.k, self.v, self.k_storage, self.v_storage = pool
            n_pages = self.k.size(0)
            perm = np.random.default_rng(seed).permutation(n_pages)[used:]
            assert len(perm) >= sum(npp) + SPARE and self.k.size(2) == P
        else:
            n_pages = sum(npp) + SPARE
            perm = np.random.default_rng(seed).permutation(n_pages)
            self.k_storage, self.v_storage = storages
            self.kb = PU.new_backing(n_pages, H, P, D, dtype, storages[0])
            self.vb = PU.new_backing(n_pages, H, P, D, dtype, storages[1])
            self.k, self.v = PU.pool_view(self.kb, storages[0]), PU.pool_view(self.vb, storages[1])
        self.rows, at = [], 0
        full = np.full((B, max(npp + [0]) + extra), -1, dtype=np.int32)
        for b in range(B):
            self.rows.append(perm[at:at + npp[b]].astype(np.int64))
            full[b, :npp[b]] = self.rows[b]
            at += npp[b]
        self.table_np = full
        self.table = torch.from_numpy(full).to(PU.DEV)

    def paged_dest(self, k_scale=None, v_scale=None):
        from kvcompress import PagedDest
        if self.same:
            return PagedDest(self.table)
        return PagedDest(self.table, self.k, self.v, k_scale, v_scale)

    def snapshot(self):
        return self.kb.clone(), self.vb.clone()

    def expect(self, snap, k_rows, v_rows, b=None):
        """Write the expected rows (numpy [B, H, n, D], or [1, H, n, D] of sequence b) into a
        snapshot of the destination's backings through the destination table."""
        import paged_util as PU
        from gpu_util import to_dev
        for back, storage, rows in ((snap[0], self.k_storage, k_rows),
                                    (snap[1], self.v_storage, v_rows)):
            view = PU.pool_view(back, storage)
            rows = to_dev(rows, PU.DEV) if isinstance(rows, np.ndarray) else rows
            if b is None:
                for i in range(rows.shape[0]):
                    PU.write_rows(view, self.rows[i][None, :], rows[i:i + 1])
            else:
                PU.write_rows(view, self.rows[b][None, :], rows)

    def assert_pools(self, snap, ctx):
        import torch
        import paged_util as PU

        def ints(t):
            return t.view(torch.uint8) if t.element_size() == 1 else PU.ints(t)
        assert torch.equal(ints(self.kb), ints(snap[0])), ctx + ("K destination pool",)
        assert torch.equal(ints(self.vb), ints(snap[1])), ctx + ("V destination pool",)


class spare:
    """with spare(n): the pools built inside (paged_util.Layer, ragged_util.RaggedLayer,
    fp8_gpu.Pool, scaled_gpu.ScaledPool) get n more pages than they need plus the usual 7 spare
    ones: room for destination pages in the same pool.  They are the ids of the pool's seeded
    permutation behind its source pages."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        import paged_util as PU
        self.was = PU.SPARE
        PU.SPARE = self.was + self.n

    def __exit__(self, *exc):
        import paged_util as PU
        PU.SPARE = self.was


def same_pool_dest(pl, n_rows, seed, used, extra=1):
    """Fresh pages of layer pl's own pool (paged_util.Layer / ragged_util.RaggedLayer built with
    room for them; `seed` / `used`: its permutation seed and its count of source pages)."""
    return Dest(n_rows, pl.P, seed, pool=(pl.kb, pl.vb, pl.k, pl.v, pl.k_storage, pl.v_storage),
                used=used, extra=extra)


# ---------------------------------------------------------------------------------------------
# CPU: the model of the delivery
# ---------------------------------------------------------------------------------------------
def read_rows(pool, table_row, P, n):
    """Logical rows [0, n) of one sequence: pool [N, H, P, ...] -> [H, n, ...]."""
    pos = np.arange(n)
    return np.moveaxis(pool[table_row[pos // P], :, pos % P], 0, 1)


def write_rows(pool, table_row, P, rows):
    """rows [H, n, ...] -> logical rows [0, n) of one sequence of pool [N, H, P, ...]."""
    n = rows.shape[1]
    pos = np.arange(n)
    pool[table_row[pos // P], :, pos % P] = np.moveaxis(rows, 1, 0)


def deliver(pools, src_tables, P_src, dst_pools, dst_tables, P_dst, row_maps, wrong=None):
    """The model: for every sequence b with row map row_maps[b] (int array [H, n_out]: the source
    row of every output row; None: a sequence of another launch group, nothing moves), read every
    pool of `pools` (K, V and the per-token scale pools, arrays [N, H, P_src, ...]) through
    src_tables[b] and write output row t through dst_tables[b] at page size P_dst into the matching
    array of dst_pools (the same objects as `pools` for fresh pages of the same pool).  All reads
    happen before all writes (the caller's promise makes the order immaterial).

    wrong: None, or one of the four wrong engines --
      "src_table"   rows addressed through the source table;
      "src_psize"   the destination slot computed with the source page size;
      "scales_stay" scale words (pools[2:]) left behind;
      "no_passthrough" a sequence whose map is the identity over its whole length is not copied.
    `lens[b]` (for no_passthrough) is taken from the map itself: identity maps count as
    pass-through."""
    staged = []
    for b, m in enumerate(row_maps):
        if m is None:
            staged.append(None)
            continue
        n = m.shape[1]
        if wrong == "no_passthrough" and n and (m == np.arange(n)[None, :]).all():
            staged.append(None)
            continue
        per_pool = []
        for pool in pools:
            src = read_rows(pool, src_tables[b], P_src, int(m.max()) + 1 if n else 0)
            idx = m.reshape(m.shape + (1,) * (src.ndim - 2))
            per_pool.append(np.take_along_axis(src, idx, axis=1) if n else src[:, :0])
        staged.append(per_pool)
    for b, per_pool in enumerate(staged):
        if per_pool is None:
            continue
        for i, (rows, dst) in enumerate(zip(per_pool, dst_pools)):
            if wrong == "scales_stay" and i >= 2:
                continue
            table = src_tables[b] if wrong == "src_table" else dst_tables[b]
            P = P_src if wrong == "src_psize" else P_dst
            if wrong == "src_psize":  # page and slot from the SOURCE page size (the slot folded
                n = rows.shape[1]     # back into the real page)
                pos = np.arange(n)
                page = table[np.minimum(pos // P, len(table) - 1)]  # (a table read clamped)
                dst[page, :, (pos % P) % P_dst] = np.moveaxis(rows, 1, 0)
            else:
                write_rows(dst, table, P, rows)
