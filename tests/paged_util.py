"""Page pools for the paged-cache GPU tests (tests/test_paged_gpu.py, tests/test_paged_graph.py).

A pool has 7 spare pages, is poison-filled and is addressed through a seeded permutation of page
ids; each batch row gets its own pages.  By default K pools are stored [N, H, P, D] and V pools
[N, P, H, D], so their stride triples differ (Layer's k_storage / v_storage choose otherwise).
Both are handed to the engine as [N, H, P, D] views.  Checks compare the WHOLE backing buffer with
a snapshot that has the expected rows written in through the table: the result and every byte
that must not change in one comparison.
"""
import numpy as np
import torch

from gpu_util import to_dev

DEV = "cuda:0"
SPARE = 7
POISON = 0x5A
INT = {2: torch.int16, 4: torch.int32}


def ints(t):
    return t.view(INT[t.element_size()])


def pool_view(back, storage):
    """The [N, H, P, D] view of a backing buffer stored `storage`."""
    return back if storage == "nhpd" else back.permute(0, 2, 1, 3)


def new_backing(n_pages, H, P, D, dtype, storage):
    shape = (n_pages, H, P, D) if storage == "nhpd" else (n_pages, P, H, D)
    back = torch.empty(shape, dtype=dtype, device=DEV)
    back.view(torch.uint8).fill_(POISON)
    return back


def page_table(B, S, P, seed, n_pages=None):
    """(int64 numpy table [B, ceil(S / P)] of distinct ids from a seeded permutation, pool size)."""
    npp = -(-S // P)
    n_pages = B * npp + SPARE if n_pages is None else n_pages
    perm = np.random.default_rng(seed).permutation(n_pages)
    return perm[:B * npp].reshape(B, npp).astype(np.int64), n_pages


def write_rows(view, table, rows, first=0):
    """Logical rows [first, first + n) of every (b, h) <- rows [B, H, n, D], through `table`
    (a device or numpy [B, pages] table)."""
    n, P = rows.shape[2], view.shape[2]
    if n == 0:
        return
    tab = torch.as_tensor(np.asarray(table.cpu()) if isinstance(table, torch.Tensor) else table,
                          device=view.device).long()
    pos = torch.arange(first, first + n, device=view.device)
    view[tab[:, pos // P], :, pos % P] = rows.permute(0, 2, 1, 3)


class Layer:
    """One paged layer: K / V backings and views, the device block table, and the PagedKV."""

    def __init__(self, k_np, v_np, P, seed, table=None, n_pages=None, table_cols=None,
                 k_storage="nhpd", v_storage="nphd"):
        from kvcompress import PagedKV
        k, v = to_dev(k_np, DEV), to_dev(v_np, DEV)
        B, H, S, D = k.shape
        if table is None:
            table, n_pages = page_table(B, S, P, seed, n_pages)
        self.table_np, self.P, self.S = table, P, S
        cols = table.shape[1] if table_cols is None else table_cols
        full = np.full((B, cols), -1, dtype=np.int32)  # entries past the sequence are never read
        full[:, :table.shape[1]] = table
        self.table = torch.from_numpy(full).to(DEV)
        self.k_storage, self.v_storage = k_storage, v_storage
        self.kb = new_backing(n_pages, H, P, D, k.dtype, k_storage)
        self.vb = new_backing(n_pages, H, P, D, k.dtype, v_storage)
        self.k, self.v = pool_view(self.kb, k_storage), pool_view(self.vb, v_storage)
        assert (self.k.stride() != self.v.stride()) == (k_storage != v_storage) or H == 1 or P == 1
        write_rows(self.k, table, k)
        write_rows(self.v, table, v)
        self.paged = PagedKV(self.k, self.v, self.table, S)

    def snapshot(self):
        return self.kb.clone(), self.vb.clone()

    def expect(self, snap, k_rows, v_rows, first=0):
        """Write the expected rows (numpy, rows [first, ...)) into a snapshot through the table."""
        for back, storage, rows in ((snap[0], self.k_storage, k_rows),
                                    (snap[1], self.v_storage, v_rows)):
            write_rows(pool_view(back, storage), self.table_np, to_dev(rows, DEV), first)

    def assert_pools(self, snap, ctx):
        assert torch.equal(ints(self.kb), ints(snap[0])), ctx + ("K pool",)
        assert torch.equal(ints(self.vb), ints(snap[1])), ctx + ("V pool",)
