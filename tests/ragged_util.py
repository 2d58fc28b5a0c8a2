"""Ragged paged batches for the tests (tests/test_ragged_*.py): per-sequence inputs, pools whose
block-table rows have their own lengths, and the per-sequence oracle.

A RaggedLayer holds B sequences of different lengths in one poisoned pool with spare pages
(tests/paged_util.py's conventions): every sequence has its own pages from a seeded permutation,
and the table entries past a sequence's last page are -1 (never read).  Checks compare the WHOLE
backing buffers with a snapshot that has the expected rows written in through the table.

Expected bytes come from the CPU oracle on each sequence ALONE -- every layer restricted to
sequence b -- which is the reference method on a batch of one.
"""
import numpy as np

import prng


def gen_sequences(seed, lens, H, D, dtype, variant="normal"):
    """[(K_b, V_b)] numpy [1, H, len_b, D] per sequence (storage representation)."""
    out = []
    for b, n in enumerate(lens):
        shape = (1, H, n, D)
        out.append((prng.gen_keys(seed + 101 * b, shape, dtype, variant),
                    prng.gen_values(seed + 101 * b, shape, dtype)))
    return out


def oracle_per_sequence(method, kw, layers_np):
    """layers_np[l][b] = (K, V).  Returns ref[l][b] = (K_out, V_out, kind) of the oracle method run
    on sequence b's layers alone."""
    from oracle import oracle
    L, B = len(layers_np), len(layers_np[0])
    ref = [[None] * B for _ in range(L)]
    for b in range(B):
        out = oracle.METHODS[method]([layers_np[l][b] for l in range(L)], **kw)
        for l in range(L):
            ref[l][b] = out[l]
    return ref


class RaggedLayer:
    """One ragged paged layer on the GPU: backings, [N, H, P, D] views, the device block table
    ([B, longest + 1 columns], -1 past each sequence) and the PagedKV with per-sequence lengths."""

    def __init__(self, seqs, P, seed, k_storage="nhpd", v_storage="nphd", lens_as=list):
        import torch
        import paged_util as PU
        from gpu_util import to_dev
        from kvcompress import PagedKV
        self.lens = [k.shape[2] for k, _ in seqs]
        B, H, D = len(seqs), seqs[0][0].shape[1], seqs[0][0].shape[3]
        npp = [-(-n // P) for n in self.lens]
        n_pages = sum(npp) + PU.SPARE
        perm = np.random.default_rng(seed).permutation(n_pages)
        self.rows, at = [], 0
        full = np.full((B, max(npp) + 1), -1, dtype=np.int32)
        for b in range(B):
            self.rows.append(perm[at:at + npp[b]].astype(np.int64))
            full[b, :npp[b]] = self.rows[b]
            at += npp[b]
        self.P, self.table_np = P, full
        self.table = torch.from_numpy(full).to(PU.DEV)
        self.k_storage, self.v_storage = k_storage, v_storage
        dtype = to_dev(seqs[0][0][:, :, :0], PU.DEV).dtype
        self.kb = PU.new_backing(n_pages, H, P, D, dtype, k_storage)
        self.vb = PU.new_backing(n_pages, H, P, D, dtype, v_storage)
        self.k, self.v = PU.pool_view(self.kb, k_storage), PU.pool_view(self.vb, v_storage)
        self.fill(seqs)
        self.paged = PagedKV(self.k, self.v, self.table, lens_as(self.lens))

    def fill(self, seqs):
        """(Re)write every sequence's rows; the rest of the pools becomes poison again."""
        import torch
        import paged_util as PU
        from gpu_util import to_dev
        self.kb.view(torch.uint8).fill_(PU.POISON)
        self.vb.view(torch.uint8).fill_(PU.POISON)
        for b, (k, v) in enumerate(seqs):
            PU.write_rows(self.k, self.rows[b][None, :], to_dev(k, PU.DEV))
            PU.write_rows(self.v, self.rows[b][None, :], to_dev(v, PU.DEV))

    def snapshot(self):
        return self.kb.clone(), self.vb.clone()

    def expect(self, snap, b, k_rows, v_rows, first=0):
        """Write sequence b's expected rows (numpy, rows [first, ...)) into a snapshot."""
        import paged_util as PU
        from gpu_util import to_dev
        for back, storage, rows in ((snap[0], self.k_storage, k_rows),
                                    (snap[1], self.v_storage, v_rows)):
            PU.write_rows(PU.pool_view(back, storage), self.rows[b][None, :],
                          to_dev(rows, PU.DEV), first)

    def assert_pools(self, snap, ctx):
        import torch
        import paged_util as PU
        assert torch.equal(PU.ints(self.kb), PU.ints(snap[0])), ctx + ("K pool",)
        assert torch.equal(PU.ints(self.vb), PU.ints(snap[1])), ctx + ("V pool",)


def build(seed, lens, H, D, dtype, P, n_layers, variant="normal", storages=("nhpd", "nphd"),
          lens_as=list):
    """(layers_np[l][b], [RaggedLayer]) of n_layers layers over the same lengths."""
    layers_np = [gen_sequences(seed + 1000 * l, lens, H, D, dtype, variant)
                 for l in range(n_layers)]
    pls = [RaggedLayer(layers_np[l], P, seed + 7 * l, *storages, lens_as=lens_as)
           for l in range(n_layers)]
    return layers_np, pls


def check_against_oracle(method, kw, layers_np, pls, ctx):
    """Run compress_paged on the ragged layers and compare lengths and whole pools with the
    per-sequence oracle."""
    import torch
    from kvcompress import compress_paged
    ref = oracle_per_sequence(method, kw, layers_np)
    snaps = [pl.snapshot() for pl in pls]
    before = [pl.snapshot() for pl in pls]
    lens = compress_paged(method, [pl.paged for pl in pls], **kw)
    torch.cuda.synchronize()
    assert len(lens) == len(pls), ctx
    for l, (pl, snap) in enumerate(zip(pls, snaps)):
        want = [ref[l][b][0].shape[2] for b in range(len(pl.lens))]
        assert list(lens[l]) == want, ctx + (l, "lengths", lens[l], want)
        moved = False
        for b in range(len(pl.lens)):
            rk, rv, kind = ref[l][b]
            if kind != "same":
                pl.expect(snap, b, rk, rv)
                moved |= rk.shape[2] > 0
        pl.assert_pools(snap, ctx + (l,))
        if moved:  # the expectation is not the untouched pool
            import paged_util as PU
            assert not torch.equal(PU.ints(pl.kb), PU.ints(before[l][0])), ctx + (l, "unchanged")
    return lens, ref


# ---- the every-method cases (GPU test 1) and their CPU power test --------------------------------
LENS = [0, 37, 512, 513, 1500]
H = 2
METHOD_CASES = [
    ("fix_size_l2", dict(fix_kv_size=512, keep_ratio=0.25, skip_layers=[0]), 3),
    ("l2_compress", dict(keep_ratio=0.5, prune_after=512, skip_layers=[1]), 3),
    ("streaming_llm", dict(start_size=4, recent_size=508, skip_layers=[1]), 2),
    ("recent_only", dict(window_size=512, skip_layers=[0]), 2),
    ("h2o_l2", dict(start_size=4, heavy_hitter_size=64, recent_size=444, skip_layers=[0]), 3),
    ("snapkv_lite", dict(observation_window=32, keep_size=512, skip_layers=[1]), 3),
    ("pyramid_kv", dict(base_size=512, layer_decay=0.9, min_size=64, skip_layers=[2]), 6),
    ("adaptive_l2", dict(target_size=512, soft_limit=256, hard_limit=1024, skip_layers=[0]), 2),
    ("evict_for_space", dict(num_coming=1, start_size=4, recent_size=508, skip_layers=[0]), 2),
]
GEOMETRIES = [  # (P, dtype, D, (K storage, V storage))
    (1, "bf16", 64, ("nhpd", "nphd")),
    (16, "fp16", 128, ("nphd", "nhpd")),
    (64, "fp32", 80, ("nhpd", "nhpd")),
]


# ---- the seeded sweep (GPU test 6) and its CPU floors -------------------------------------------
def sweep_cases(n=64, seed=20240):
    """n seeded random ragged calls: method and kwargs, B in 2..6, lengths in 0..2000 with one
    stratum (every eighth call) reaching above 4 096, P, dtype / D, storages."""
    rng = np.random.default_rng(seed)
    names = [m for m, _, _ in METHOD_CASES]
    cases = []
    for i in range(n):
        method = names[i % len(names)] if i < 2 * len(names) else names[rng.integers(len(names))]
        B = int(rng.integers(2, 7))
        size = int(rng.choice([64, 200, 512, 700]))
        hi = 2000
        lens = [int(x) for x in rng.integers(0, hi + 1, B)]
        at = [int(x) for x in rng.permutation(B)]
        lens[at[0]] = int(rng.integers(0, size // 2 + 1))       # short: every method passes it
        lens[at[1]] = int(rng.integers(2 * size + 40, hi + 1))  # long: every method compresses
        if i % 8 == 3:
            lens[at[-1]] = int(rng.integers(4097, 4700))
        L = int(rng.integers(2, 4))
        skip = [int(rng.integers(L))] if rng.integers(2) else []
        kw = {
            "fix_size_l2": dict(fix_kv_size=size, keep_ratio=float(rng.choice([0.0, 0.25, 0.5])),
                                strategy=str(rng.choice(["keep_low", "keep_high"])),
                                skip_layers=skip),
            "l2_compress": dict(keep_ratio=float(rng.choice([0.3, 0.5, 0.9])), prune_after=size,
                                skip_layers=skip),
            "streaming_llm": dict(start_size=4, recent_size=size - 4, skip_layers=skip),
            "recent_only": dict(window_size=size, skip_layers=skip),
            "h2o_l2": dict(start_size=4, heavy_hitter_size=size // 4,
                           recent_size=size - 4 - size // 4, skip_layers=skip),
            "snapkv_lite": dict(observation_window=int(rng.choice([8, 32])), keep_size=size,
                                pooling_kernel=int(rng.choice([1, 5, 7])), skip_layers=skip),
            "pyramid_kv": dict(base_size=size, layer_decay=0.8, min_size=32, skip_layers=skip),
            "adaptive_l2": dict(target_size=size, soft_limit=size // 2, hard_limit=2 * size,
                                skip_layers=skip),
            "evict_for_space": dict(num_coming=int(rng.integers(1, 4)), start_size=4,
                                    recent_size=size - 4, skip_layers=skip),
        }[method]
        P, dtype, D, st = GEOMETRIES[int(rng.integers(len(GEOMETRIES)))]
        P = int(rng.choice([1, 4, 16, 64, 256]))
        st = tuple(str(s) for s in rng.choice(["nhpd", "nphd"], 2))
        cases.append(dict(id=f"{i:02d}-{method}", method=method, kw=kw, lens=lens, L=L, P=P,
                          dtype=dtype, D=D, storages=st, H=int(rng.integers(1, 3)),
                          variant=str(rng.choice(["normal", "few"])), seed=seed + 31 * i))
    return cases
