"""What causal attention column sums cost ("Attention column sums"): 32
layers of [1, 32, 16384, 128] bf16 at q = 1, 32, 512 and 16 384.  In one process, alternating over
`--rounds` rounds, per q:
  colsum_ms      the kvc_colsum_score launch set alone (statistics, lse merge, column sums), `reps`
                 launches between two device events, per launch;
  colsum_lse_ms  the same with a caller's lse (the column-sum kernel alone);
  call_ms        the whole H2OAttentionManager.update_from_queries call (checks, plan,
                 allocations, the sums, kvc_attn_accumulate);
  torch_ms       matmul -> masked softmax -> sum per layer on the same GPU, where torch can hold
                 the logits (q <= 512);
  observe_ms     q = 32 only: the kvc_observe_score set of the same build over the same K and Q
                 (W = 32, G = 1, pooling_kernel = 1), and colsum_vs_observe = colsum_ms / observe_ms.
Medians with [min, max].  GPU box only.

  python tools/colsum_bench.py [--layers 32] [--seq 16384] [--heads 32] [--q 1,32,512,16384]
                               [--rounds 5] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs3602-llm-inference-acceleration_amd"))
from kvcompress import _engine as E  # noqa: E402
from kvcompress import _native as N  # noqa: E402
from kvcompress.methods.h2o_attention import H2OAttentionManager  # noqa: E402

DEV = torch.device("cuda:0")
D = 128


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def colsum_set(ks, qs, lses):
    """The planned kvc_colsum_score launch set (bf16 rows out) as a callable."""
    (_, H, S, _), ql = ks[0].shape, qs[0].shape[2]
    outs = [torch.empty(1, H, S, dtype=torch.bfloat16, device=DEV) for _ in ks]
    table = np.zeros(len(ks), dtype=N.COLSUM_LAYER_DTYPE)
    for i, (k, q, o) in enumerate(zip(ks, qs, outs)):
        table[i] = (k.data_ptr(), k.stride()[:3], q.data_ptr(), q.stride()[:3],
                    lses[i].data_ptr() if lses else 0, 0, o.data_ptr(), S, S, ql, 0)
    p = N.ColsumParams(dtype=N.KVC_BF16, batch=1, heads=H, q_heads=H, head_dim=D)
    rc, nbytes = N.colsum_plan(p, table)
    N.check(rc, "kvc_colsum_plan")
    scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        N.check(N.colsum_score(p, table, scratch.data_ptr(), nbytes, stream), "kvc_colsum_score")
    run.keep, run.scratch_bytes = (outs, table, p, scratch), nbytes
    return run


def observe_set(ks, qs):
    """kvc_observe_score over the same K and Q (q = W = 32, G = 1, no pooling, zone = the prefix)."""
    (_, H, S, _), W = ks[0].shape, 32
    jobs = [E.Segments(i, k, k, zone_len=S - W, n_select=64, tail_start=S - W, tail_len=W)
            for i, k in enumerate(ks)]
    p = E._params(torch.bfloat16, 1, H, D, N.KVC_DESC, N.KVC_ALGO_TOPK, False)
    built = E._build_table(0, torch.bfloat16, 1, H, D, jobs)
    table = built[0]
    rc, info = N.plan(p, table)
    N.check(rc, "kvc_plan")
    otable = np.zeros(len(ks), dtype=N.OBSERVE_LAYER_DTYPE)
    for i, q in enumerate(qs):
        otable[i] = (q.data_ptr(), q.stride()[:3], 0)
    op = N.ObserveParams(q_heads=H, window=W, pool_kernel=1, pool_mode=N.OBS_POOL_AVG)
    rc, sbytes = N.observe_plan(p, op, table, otable)
    N.check(rc, "kvc_observe_plan")
    ws = torch.empty(int(info.workspace_bytes), dtype=torch.uint8, device=DEV)
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        N.check(N.observe_score(p, op, table, otable, ws.data_ptr(), int(info.workspace_bytes),
                                scratch.data_ptr(), sbytes, None, stream), "kvc_observe_score")
    run.keep = (built, otable, op, p, ws, scratch)
    return run


def torch_sums(ks, qs):
    out = []
    for k, q in zip(ks, qs):
        S, ql = k.shape[2], q.shape[2]
        s = torch.matmul(q, k.transpose(2, 3)).float() * D ** -0.5
        i = torch.arange(ql, device=DEV)
        s.masked_fill_(torch.arange(S, device=DEV)[None, :] > (S - ql + i)[:, None], float("-inf"))
        out.append(torch.softmax(s, -1).sum(2))
    return out


def point(L, S, H, ql, rounds, reps, gen):
    ks = [torch.empty(1, H, S, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
          for _ in range(L)]
    qs = [torch.empty(1, H, ql, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
          for _ in range(L)]
    # any finite lse gives the column-sum kernel its full work (the sums are then not probabilities)
    lses = [torch.full((1, H, ql), 12.0, dtype=torch.float32, device=DEV) for _ in range(L)]
    mgr = H2OAttentionManager(num_layers=L, num_heads=H)

    def call():
        mgr.reset()
        mgr.update_from_queries(qs, ks)

    stats = colsum_set(ks, qs, None)
    runs = {"colsum_ms": stats, "colsum_lse_ms": colsum_set(ks, qs, lses), "call_ms": call}
    if ql <= 512:
        runs["torch_ms"] = lambda: torch_sums(ks, qs)
    if ql == 32:
        runs["observe_ms"] = observe_set(ks, qs)
    for fn in runs.values():  # warm-up: code objects, allocator pools
        fn()
    torch.cuda.synchronize()
    times = {key: [] for key in runs}
    for _ in range(rounds):  # alternating
        for key, fn in runs.items():
            times[key].append(timed(fn, 2 if key == "torch_ms" else reps))
    rec = {"layers": L, "seq": S, "heads": H, "q": ql, "rounds": rounds,
           "scratch_bytes": stats.scratch_bytes, "lib": os.path.basename(N.LIB_PATH),
           "logits_per_pass": L * H * (ql * (S - ql) + ql * (ql + 1) // 2)}
    for key, v in times.items():
        rec[key] = round(statistics.median(v), 4)
        rec[key + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    if "observe_ms" in rec:
        rec["colsum_vs_observe"] = round(rec["colsum_ms"] / rec["observe_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--seq", type=int, default=16384)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--q", default="1,32,512,16384")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    for ql in (int(x) for x in a.q.split(",")):
        line = json.dumps(point(a.layers, a.seq, a.heads, min(ql, a.seq), a.rounds,
                                a.reps if ql <= 4096 else 1, gen))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
