"""GPU-side helpers of the scaled fp8 suites: fp8_gpu's page pools with a K and a V scale pool
beside them, and the C-ABI launcher for kvc_plan_scaled / kvc_launch_scaled.

A scale pool is an int32 backing (torch indexes it everywhere; the engine gets a float32 VIEW)
stored [N, H, P + 3] or [N, P, H + 3] and handed over as the [N, H, P] view of its leading
columns: strided both ways, with poison-filled padding between the rows that no launch may touch.
Checks compare WHOLE backings -- K, V, K scales, V scales -- with a snapshot that has the expected
rows and scale words written in through the table."""
import numpy as np
import torch

import fp8_gpu as G
import paged_util as PU
from kvcompress import _native as N

DEV = G.DEV
PAD = 3
SCALE_STORAGES = (("nhp", "nph"), ("nph", "nhp"))


def scale_backing(n_pages, H, P, storage):
    shape = (n_pages, H, P + PAD) if storage == "nhp" else (n_pages, P, H + PAD)
    back = torch.empty(shape, dtype=torch.int32, device=DEV)
    back.view(torch.uint8).fill_(PU.POISON)
    return back


def scale_view(back, storage, H, P):
    """The [N, H, P] int32 view of a scale backing."""
    return back[:, :, :P] if storage == "nhp" else back[:, :, :H].permute(0, 2, 1)


def write_words(view, pages, w, first=0):
    """Scale words of logical rows [first, first + n) of every (b, h) <- w [B, H, n] (numpy uint32
    or float32), through the int64 page rows `pages` [B, pages]."""
    w = np.ascontiguousarray(w)
    n, P = w.shape[2], view.shape[2]
    if n == 0:
        return
    tab = torch.as_tensor(pages, device=view.device).long()
    pos = torch.arange(first, first + n, device=view.device)
    view[tab[:, pos // P], :, pos % P] = torch.from_numpy(w.view(np.int32)).to(DEV).permute(0, 2, 1)


class ScaledPool(G.Pool):
    """fp8_gpu.Pool of sequences (k8, v8, ks, vs) -- numpy [1, H, len_b, D] bytes and [1, H, len_b]
    float32 scales -- with the K and V scale pools.  k_mode / v_mode: "pool" (per-token scales),
    "uniform" (one float, the middle word of a poisoned 3-word buffer) or "none"."""

    def __init__(self, seqs, fmt, P, seed, storages=G.STORAGES[0], scale_storages=SCALE_STORAGES[0],
                 k_mode="pool", v_mode="pool", uniform=(None, None)):
        super().__init__([(k, v) for k, v, _, _ in seqs], fmt, P, seed, storages)
        H, n_pages = seqs[0][0].shape[1], self.kb.shape[0]
        self.H = H
        self.scale_storages, self.modes = scale_storages, (k_mode, v_mode)
        self.sb, self.sv = [], []   # backings and the tensors handed to the engine
        for side, mode in enumerate(self.modes):
            if mode == "pool":
                back = scale_backing(n_pages, H, P, scale_storages[side])
                view = scale_view(back, scale_storages[side], H, P)
                for b, sq in enumerate(seqs):
                    write_words(view, self.rows[b][None, :], sq[2 + side])
                self.sb.append(back)
                self.sv.append(view.view(torch.float32))
            elif mode == "uniform":
                back = torch.empty(3, dtype=torch.int32, device=DEV)
                back.view(torch.uint8).fill_(PU.POISON)
                back[1:2].view(torch.float32).fill_(uniform[side])
                self.sb.append(back)
                self.sv.append(back[1:2].view(torch.float32))
            else:
                self.sb.append(None)
                self.sv.append(None)

    def paged(self, ragged=False):
        from kvcompress import PagedKV
        return PagedKV(self.k, self.v, self.table, list(self.lens) if ragged else self.lens[0],
                       k_scale=self.sv[0], v_scale=self.sv[1])

    def scales_row(self):
        """The pool's kvc_scales_t, built here (not by PagedKV)."""
        z = np.zeros(1, dtype=N.SCALES_DTYPE)
        flags = 0
        for side, (name, uni, none) in enumerate((("k", N.SCALE_K_UNIFORM, N.SCALE_K_NONE),
                                                  ("v", N.SCALE_V_UNIFORM, N.SCALE_V_NONE))):
            t, mode = self.sv[side], self.modes[side]
            if mode == "none":
                flags |= none
                continue
            z[0][name + "_scale"] = t.data_ptr()
            if mode == "uniform":
                flags |= uni
            else:
                z[0][name + "_page_stride"] = t.stride(0)
                z[0][name + "_stride"] = (t.stride(1), t.stride(2))
        z[0]["flags"] = flags
        return z

    def snapshot(self):
        return (self.kb.clone(), self.vb.clone()) + tuple(
            None if b is None else b.clone() for b in self.sb)

    def expect(self, snap, b, k_rows, v_rows, wk=None, wv=None, first=0):
        super().expect(snap, b, k_rows, v_rows, first)
        for side, w in enumerate((wk, wv)):
            if self.modes[side] == "pool":
                view = scale_view(snap[2 + side], self.scale_storages[side], self.H, self.P)
                write_words(view, self.rows[b][None, :], w, first)

    def assert_pools(self, snap, ctx):
        super().assert_pools(snap, ctx)
        for side, name in enumerate(("K scales", "V scales")):
            if self.sb[side] is not None:
                assert torch.equal(self.sb[side], snap[2 + side]), ctx + (name,)

    def changed(self, snap):
        """Which of the four backings differ from `snap`."""
        backs = (self.kb, self.vb) + tuple(self.sb)
        return [b is not None and not torch.equal(b, s) for b, s in zip(backs, snap)]


class Launch(G.Launch):
    """fp8_gpu.Launch through kvc_plan_scaled / kvc_launch_scaled."""

    def __init__(self, dtype, B, H, D, order, algo, table, pages, scales, ragged=None, flags=0,
                 external=0):
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.p = N.Params(dtype=dtype, batch=B, heads=H, head_dim=D, order=order, algo=algo,
                          phases=N.PHASE_GATHER if external else N.PHASE_ALL,
                          external_index=external, flags=flags,
                          device_status=self.status.data_ptr())
        self.table, self.pages, self.ragged, self.scales = table, pages, ragged, scales
        rc, self.info = N.plan_scaled(self.p, table, pages, ragged, scales)
        assert rc == 0, rc
        self.ws = torch.full((max(int(self.info.workspace_bytes), 256),), 0xFF, dtype=torch.uint8,
                             device=DEV)

    def run(self, phases, sync=True):
        self.p.phases = phases
        rc = N.launch_scaled(self.p, self.table, self.pages, self.ragged, self.scales,
                             self.ws.data_ptr(), int(self.info.workspace_bytes),
                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        if sync:
            torch.cuda.synchronize()
            assert int(self.status.item()) == 0
