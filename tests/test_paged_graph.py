"""Graph capture of a paged decode step: the block table is device data read
when the kernels run, so a replay follows the table's CURRENT contents.

The in-place step -- 4 layers of [1, 4, 513, 64], pages of 16 tokens, fix_size_l2(512) -- is
captured after one eager warm-up call and replayed three times; before every replay the pools are
poisoned and refilled with another seeded fill and the table TENSORS are overwritten (copy_: the
pointers stay) with a new page permutation.  Every replay must equal the CPU oracle for its fill,
written through its table, in the whole pool."""
import numpy as np
import pytest
import torch

import paged_util as PU
import prng
from gpu_util import to_dev

pytestmark = pytest.mark.gpu

L, B, H, S, D, P = 4, 1, 4, 513, 64, 16
KW = dict(fix_kv_size=512, keep_ratio=0.0, skip_layers=[])


def test_captured_in_place_decode_step_follows_the_table():
    from kvcompress import PagedKV, compress_paged
    from oracle import oracle
    npp = -(-S // P)
    n_pages = B * npp + PU.SPARE
    backs = [(PU.new_backing(n_pages, H, P, D, torch.bfloat16, "nhpd"),
              PU.new_backing(n_pages, H, P, D, torch.bfloat16, "nphd")) for _ in range(L)]
    tables = [torch.zeros((B, npp), dtype=torch.int32, device=PU.DEV) for _ in range(L)]
    paged = [PagedKV(PU.pool_view(kb, "nhpd"), PU.pool_view(vb, "nphd"), t, S)
             for (kb, vb), t in zip(backs, tables)]

    def fill(f):
        """Poison, new permutation, new data; returns [(table, k, v)] numpy."""
        out = []
        for li, ((kb, vb), t) in enumerate(zip(backs, tables)):
            seed = 48000 + 10 * f + li
            tab, _ = PU.page_table(B, S, P, seed)
            k = prng.gen_keys(seed, (B, H, S, D), "bf16")
            v = prng.encode_positions((B, H, S, D), "bf16")
            t.copy_(torch.from_numpy(tab.astype(np.int32)))
            for back, storage, x in ((kb, "nhpd", k), (vb, "nphd", v)):
                back.view(torch.uint8).fill_(PU.POISON)
                PU.write_rows(PU.pool_view(back, storage), tab, to_dev(x, PU.DEV))
            out.append((tab, k, v))
        return out

    def check(state, what):
        torch.cuda.synchronize()
        ref = oracle.METHODS["fix_size_l2"]([(k, v) for _, k, v in state], **KW)
        for li, ((tab, k, v), (rk, rv, kind), (kb, vb)) in enumerate(zip(state, ref, backs)):
            assert kind == "new" and rk.shape[2] == 512
            for back, storage, x, r in ((kb, "nhpd", k, rk), (vb, "nphd", v, rv)):
                want = PU.new_backing(n_pages, H, P, D, torch.bfloat16, storage)
                PU.write_rows(PU.pool_view(want, storage), tab, to_dev(x, PU.DEV))
                PU.write_rows(PU.pool_view(want, storage), tab, to_dev(r, PU.DEV))
                assert torch.equal(PU.ints(back), PU.ints(want)), (what, li, storage)

    state = fill(0)
    assert compress_paged("fix_size_l2", paged, **KW) == [512] * L  # the warm-up
    check(state, "eager")
    state = fill(1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lens = compress_paged("fix_size_l2", paged, **KW)
    assert lens == [512] * L
    perms = set()
    for rep in (1, 2, 3):
        state = fill(rep)
        perms.add(tuple(state[0][0].reshape(-1)))
        g.replay()
        check(state, f"replay {rep}")
    assert len(perms) == 3
    del g  # the graph goes before the test ends, and the device is idle
    torch.cuda.synchronize()
