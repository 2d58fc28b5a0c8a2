"""GPU-side helpers of the fp8 suites: device tensors from uint8 bit patterns, page pools kept as
uint8 backings (torch indexes uint8 everywhere; the engine gets float8 VIEWS of them), and one
C-ABI launcher for dense, paged and ragged tables.  Conventions of tests/paged_util.py: poisoned
pools with spare pages behind a shuffled table, whole-buffer comparisons."""
import numpy as np
import torch

import fp8_util as F
import paged_util as PU
from kvcompress import _native as N

DEV = PU.DEV
KVC = {"e4m3": N.KVC_F8E4M3, "e5m2": N.KVC_F8E5M2}
STORAGES = (("nhpd", "nphd"), ("nphd", "nhpd"))


def dev8(a8, fmt):
    """uint8 numpy -> float8 device tensor."""
    return F.to_dev(a8, fmt, DEV)


def as_u8(t):
    return t.view(torch.uint8)


class Pool:
    """B sequences (numpy uint8 [1, H, len_b, D] K / V pairs, or one [B, H, S, D] pair) in
    poisoned K / V page pools; .k / .v are the float8 [N, H, P, D] views the engine takes."""

    def __init__(self, seqs, fmt, P, seed, storages=STORAGES[0]):
        if isinstance(seqs, tuple):  # one dense [B, H, S, D] pair: B equally long sequences
            k, v = seqs
            seqs = [(k[b:b + 1], v[b:b + 1]) for b in range(k.shape[0])]
        self.fmt, self.P, self.lens = fmt, P, [k.shape[2] for k, _ in seqs]
        B, H, D = len(seqs), seqs[0][0].shape[1], seqs[0][0].shape[3]
        npp = [-(-n // P) for n in self.lens]
        n_pages = sum(npp) + PU.SPARE
        perm = np.random.default_rng(seed).permutation(n_pages)
        full = np.full((B, max(npp + [0]) + 1), -1, dtype=np.int32)
        self.rows, at = [], 0
        for b in range(B):
            self.rows.append(perm[at:at + npp[b]].astype(np.int64))
            full[b, :npp[b]] = self.rows[b]
            at += npp[b]
        self.table = torch.from_numpy(full).to(DEV)
        self.storages = storages
        self.kb = PU.new_backing(n_pages, H, P, D, torch.uint8, storages[0])
        self.vb = PU.new_backing(n_pages, H, P, D, torch.uint8, storages[1])
        self.k8 = PU.pool_view(self.kb, storages[0])
        self.v8 = PU.pool_view(self.vb, storages[1])
        for b, (k, v) in enumerate(seqs):
            self.write(self.k8, b, k)
            self.write(self.v8, b, v)
        t8 = F.torch_dtype(fmt)
        self.k, self.v = self.k8.view(t8), self.v8.view(t8)

    def write(self, view8, b, rows, first=0):
        PU.write_rows(view8, self.rows[b][None, :], torch.from_numpy(np.ascontiguousarray(rows))
                      .to(DEV), first)

    def paged(self, ragged=False):
        from kvcompress import PagedKV
        return PagedKV(self.k, self.v, self.table, list(self.lens) if ragged else self.lens[0])

    def snapshot(self):
        return self.kb.clone(), self.vb.clone()

    def expect(self, snap, b, k_rows, v_rows, first=0):
        self.write(PU.pool_view(snap[0], self.storages[0]), b, k_rows, first)
        self.write(PU.pool_view(snap[1], self.storages[1]), b, v_rows, first)

    def assert_pools(self, snap, ctx):
        assert torch.equal(self.kb, snap[0]), ctx + ("K pool",)
        assert torch.equal(self.vb, snap[1]), ctx + ("V pool",)


def layer_row(s, S, k=None, v=None, ko=None, vo=None, pool=None):
    """One kvc_layer_t of phase_tables spec `s` on dense tensors k / v or on a Pool."""
    t = np.zeros(1, dtype=N.LAYER_DTYPE)[0]
    if pool is None:
        t["k"], t["v"] = k.data_ptr(), v.data_ptr()
        t["k_stride"], t["v_stride"] = k.stride()[:3], v.stride()[:3]
    else:
        t["k"], t["v"] = pool.k.data_ptr(), pool.v.data_ptr()
        t["k_stride"] = (0,) + tuple(pool.k.stride()[1:3])
        t["v_stride"] = (0,) + tuple(pool.v.stride()[1:3])
    t["k_out"] = ko.data_ptr() if ko is not None else t["k"]
    t["v_out"] = vo.data_ptr() if vo is not None else t["v"]
    t["seq_len"], t["zone_start"], t["zone_len"] = S, s["zone_start"], s["zone_len"]
    t["n_select"], t["sink_len"] = s["n_select"], s["sink"]
    t["tail_start"], t["tail_len"] = s["tail_start"], s["tail_len"]
    t["score_mode"], t["pool_kernel"] = s["score_mode"], s["pool"]
    return t


def pages_row(pool, in_place=0):
    pg = np.zeros(1, dtype=N.PAGES_DTYPE)
    pg[0] = (pool.table.data_ptr(), pool.table.stride(0), pool.k.stride(0), pool.v.stride(0),
             pool.P, pool.k.size(0), in_place, 0)
    return pg


def seq_records(specs):
    """(host SEQ_DTYPE array, its device copy) of per-sequence phase_tables specs (S in s["S"])."""
    seqs = np.zeros(len(specs), dtype=N.SEQ_DTYPE)
    for i, s in enumerate(specs):
        n_out = s["sink"] + s["n_select"] + s["tail_len"]
        seqs[i] = (s["S"], s["zone_start"], s["zone_len"], s["n_select"], s["sink"],
                   s["tail_start"], s["tail_len"], s["score_mode"], s["pool"], n_out, (0, 0))
    dev = torch.from_numpy(seqs.view(np.uint8).copy()).to(DEV)
    assert dev.data_ptr() % 16 == 0
    return seqs, dev


class Launch:
    """A planned table on a 0xFF-filled workspace with a status word of its own; run(phases)
    launches, regions() returns the norm rows and tile maxima as bytes."""

    def __init__(self, dtype, B, H, D, order, algo, table, pages=None, dests=None, ragged=None,
                 flags=0, external=0):
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.p = N.Params(dtype=dtype, batch=B, heads=H, head_dim=D, order=order, algo=algo,
                          phases=N.PHASE_GATHER if external else N.PHASE_ALL,
                          external_index=external, flags=flags,
                          device_status=self.status.data_ptr())
        self.table, self.pages, self.dests, self.ragged = table, pages, dests, ragged
        if ragged is not None:
            rc, self.info = N.plan_ragged(self.p, table, pages, ragged)
        else:
            rc, self.info = N.plan_paged(self.p, table, pages, dests)
        assert rc == 0, rc
        self.ws = torch.full((max(int(self.info.workspace_bytes), 256),), 0xFF, dtype=torch.uint8,
                             device=DEV)

    def run(self, phases, sync=True):
        """sync=False: launch only (inside a graph capture; read .status after the replays)."""
        self.p.phases = phases
        args = (self.ws.data_ptr(), int(self.info.workspace_bytes),
                torch.cuda.current_stream().cuda_stream)
        if self.ragged is not None:
            rc = N.launch_ragged(self.p, self.table, self.pages, self.ragged, *args)
        else:
            rc = N.launch_paged(self.p, self.table, self.pages, self.dests, *args)
        assert rc == 0, rc
        if sync:
            torch.cuda.synchronize()
            assert int(self.status.item()) == 0

    def regions(self):
        """(norm region [rows, norm_row_stride] uint16, tile maxima [rows, tiles] uint32): fp8 calls
        score in bf16."""
        i = self.info
        rows, ns, istr = int(i.rows), int(i.norm_row_stride), int(i.index_row_stride)
        w = self.ws.cpu().numpy()
        norms = w[i.norm_offset:i.norm_offset + rows * ns * 2].view(np.uint16).reshape(rows, ns)
        toff = (i.index_offset + rows * istr * 4 + 255) // 256 * 256  # csrc/kvc.hip tmax_offset
        assert ns <= 16384  # (no long-zone scratch between the index region and the maxima)
        tmax = w[toff:toff + rows * (ns // 64) * 4].view(np.uint32).reshape(rows, ns // 64)
        return norms.copy(), tmax.copy()

    def indices(self):
        i = self.info
        rows, istr = int(i.rows), int(i.index_row_stride)
        w = self.ws.cpu().numpy()
        return w[i.index_offset:i.index_offset + rows * istr * 4].view(np.int32).reshape(rows, istr)
