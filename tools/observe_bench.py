"""What the observation-window score costs ("Observation-window scores"):
32 layers of [1, Hkv, 16384, 128] bf16 with W = 32, keep 512, for Hkv = 32 (G = 1, the headline
geometry) and Hkv = 8 with G = 4 (one GQA point, 32 query heads).  In one process, alternating
over `--rounds` rounds, per geometry:
  observe_ms   the kvc_observe_score launch set alone (three kernels), `reps` launches between
               two device events, per launch;
  score_ms     the existing SCORE kernel (key norms) over the same keys: the bytes-equivalent
               floor, one read of K;
  call_ms      the whole snapkv_compress call (plan, observe, SELECT | GATHER, allocations);
  torch_ms     the same scores outside HIP: matmul -> masked softmax -> sum -> avg_pool1d per layer.
`read_rate_vs_score` = score_ms / (observe_ms / 2): the rate at which each of the two passes
reads K, as a fraction of SCORE's; above 1 the second pass was served from cache.
KVC_LIB=<variant libkvc.so> measures a variant build (e.g. non-temporal pass-2 loads).

--sources: what a block table and fp8 keys cost the same kernels (kvc_observe_score_paged).  Per
geometry and source -- paged bf16 pools stored [N, P, H, D] behind shuffled tables at P = 16 and
P = 128, and dense e4m3 keys -- one line with the source's observe set and whole call
(snapkv_compress_paged / snapkv_compress) next to the dense bf16 set and call of the same build,
alternating in one process: medians and ranges over `--rounds` rounds, and the ratios.  A paged
call compacts in place, so from its second run on it ranks the rows its first run left: the
kernels' work does not depend on the data.

--wide: wide query groups (csrc/kvc_observe_wide.h).  32 layers of [1, 8, 16384, 128] bf16 at
W = 32 with G = 8 (Hq = 64) and, the uneven point, G = 7 (Hq = 56): the observe set and the whole
snapkv_compress call next to the query heads split into admitted groups (observation_scores at
pooling_kernel = 1 per group, added and pooled in torch) and the torch line, alternating.
GPU box only.

  python tools/observe_bench.py [--layers 32] [--seq 16384] [--rounds 5] [--reps 10] [--out FILE]
                                [--sources | --wide]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs3602-llm-inference-acceleration_amd"))
from kvcompress import _engine as E  # noqa: E402
from kvcompress import _native as N  # noqa: E402
from kvcompress import PagedKV, observation_scores, snapkv_compress, snapkv_compress_paged  # noqa: E402,E501
from kvcompress.methods.snapkv import _paged_table  # noqa: E402

DEV = torch.device("cuda:0")
D, W, KEEP, POOL = 128, 32, 512, 5


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def torch_scores(kv, qs, G):
    out = []
    for (k, _), q in zip(kv, qs):
        B, H, S, _ = k.shape
        s = torch.matmul(q.view(B, H, G * W, D), k.transpose(2, 3)).float() * D ** -0.5
        i = torch.arange(W, device=DEV).repeat(G)
        s.masked_fill_(torch.arange(S, device=DEV)[None, :] > (S - W + i)[:, None], float("-inf"))
        imp = torch.softmax(s, -1).sum(2)[:, :, :S - W]
        out.append(F.avg_pool1d(imp, POOL, 1, POOL // 2))
    return out


def geometry(name, L, S, Hkv, G, rounds, reps, gen):
    kv = [tuple(torch.empty(1, Hkv, S, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
                for _ in range(2)) for _ in range(L)]
    qs = [torch.empty(1, G * Hkv, W, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
          for _ in range(L)]
    # the launch set alone: the table snapkv_compress would plan, launched by hand
    jobs = [E.Segments(i, k, v, zone_len=S - W, n_select=KEEP - W, tail_start=S - W, tail_len=W)
            for i, (k, v) in enumerate(kv)]
    p = E._params(torch.bfloat16, 1, Hkv, D, N.KVC_DESC, N.KVC_ALGO_TOPK, False)
    table, kos, vos, _ = E._build_table(0, torch.bfloat16, 1, Hkv, D, jobs)
    rc, info = N.plan(p, table)
    N.check(rc, "kvc_plan")
    otable = np.zeros(L, dtype=N.OBSERVE_LAYER_DTYPE)
    for i, q in enumerate(qs):
        otable[i] = (q.data_ptr(), q.stride()[:3], 0)
    op = N.ObserveParams(q_heads=G * Hkv, window=W, pool_kernel=POOL, pool_mode=N.OBS_POOL_AVG)
    rc, sbytes = N.observe_plan(p, op, table, otable)
    N.check(rc, "kvc_observe_plan")
    ws = torch.empty(int(info.workspace_bytes), dtype=torch.uint8, device=DEV)
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def observe():
        N.check(N.observe_score(p, op, table, otable, ws.data_ptr(), int(info.workspace_bytes),
                                scratch.data_ptr(), sbytes, None, stream), "kvc_observe_score")

    def score():
        p.phases = N.PHASE_SCORE
        N.check(N.launch(p, table, ws.data_ptr(), int(info.workspace_bytes), stream), "kvc_launch")

    runs = {"observe_ms": observe, "score_ms": score,
            "call_ms": lambda: snapkv_compress(kv, qs, W, KEEP, POOL),
            "torch_ms": lambda: torch_scores(kv, qs, G)}
    for fn in runs.values():  # warm-up: code objects, allocator pools
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(rounds):  # alternating
        for key, fn in runs.items():
            times[key].append(timed(fn, reps if key != "torch_ms" else 2))
    rec = {"geometry": name, "layers": L, "seq": S, "kv_heads": Hkv, "group": G, "window": W,
           "k_bytes": L * Hkv * S * D * 2, "scratch_bytes": sbytes,
           "lib": os.path.basename(N.LIB_PATH)}
    for key, v in times.items():
        rec[key] = round(statistics.median(v), 4)
        rec[key + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    rec["read_rate_vs_score"] = round(rec["score_ms"] / (rec["observe_ms"] / 2), 3)
    rec["observe_gbps_two_reads"] = round(2 * rec["k_bytes"] / rec["observe_ms"] / 1e6, 1)
    return rec


def observe_set(dtype, Hkv, G, table, qs, tables=None):
    """The planned observe launch set of a table as a callable (kvc_observe_score_paged)."""
    p = E._params(dtype, 1, Hkv, D, N.KVC_DESC, N.KVC_ALGO_TOPK, False)
    ws, info = E._upload(p, table, 0, None, 1, Hkv, tables)
    otable = np.zeros(len(table), dtype=N.OBSERVE_LAYER_DTYPE)
    for i, q in enumerate(qs):
        otable[i] = (q.data_ptr(), q.stride()[:3], 0)
    op = N.ObserveParams(q_heads=G * Hkv, window=W, pool_kernel=POOL, pool_mode=N.OBS_POOL_AVG)
    pages = tables.pages if tables is not None else None
    rc, sbytes = N.observe_plan_paged(p, op, table, otable, pages)
    N.check(rc, "kvc_observe_plan_paged")
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    keep = (ws, scratch, otable, op, p, table, tables)

    def run():
        N.check(N.observe_score_paged(p, op, table, otable, pages, ws.data_ptr(),
                                      int(info.workspace_bytes), scratch.data_ptr(), sbytes, None,
                                      stream), "kvc_observe_score_paged")
    run.keep = keep
    return run


def paged_layers(kv, P, gen):
    """The layers' K / V in pools stored [N, P, H, D] behind a shuffled one-row table."""
    out = []
    for k, v in kv:
        _, H, S, _ = k.shape
        n = S // P
        perm = torch.randperm(n + 7, device=DEV, generator=gen)[:n]
        pools = []
        for x in (k, v):
            pool = torch.empty(n + 7, P, H, D, dtype=x.dtype, device=DEV)
            pool[perm] = x[0].permute(1, 0, 2).reshape(n, P, H, D)
            pools.append(pool.permute(0, 2, 1, 3))
        out.append(PagedKV(pools[0], pools[1], perm.int().view(1, n), S))
    return out


def sources(name, L, S, Hkv, G, rounds, reps, gen):
    kv = [tuple(torch.empty(1, Hkv, S, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
                for _ in range(2)) for _ in range(L)]
    qs = [torch.empty(1, G * Hkv, W, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
          for _ in range(L)]
    seg = (0, S - W, KEEP - W, 0, S - W, W)

    def dense_runs(layers):
        jobs = [E.Segments(i, k, v, zone_len=S - W, n_select=KEEP - W, tail_start=S - W,
                           tail_len=W) for i, (k, v) in enumerate(layers)]
        table = E._build_table(0, layers[0][0].dtype, 1, Hkv, D, jobs)
        run = observe_set(layers[0][0].dtype, Hkv, G, table[0], qs)
        run.keep += (table,)
        return run, lambda: snapkv_compress(layers, qs, W, KEEP, POOL)

    base_obs, base_call = dense_runs(kv)
    lines = []
    for src in ("paged_p16", "paged_p128", "fp8_e4m3"):
        if src.startswith("paged"):
            pks = paged_layers(kv, int(src[7:]), gen)
            table, tables = _paged_table(pks, [seg] * L)
            obs = observe_set(torch.bfloat16, Hkv, G, table, qs, tables)
            call = lambda: snapkv_compress_paged(pks, qs, W, KEEP, POOL)  # noqa: E731
        else:
            kv8 = [(k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)) for k, v in kv]
            obs, call = dense_runs(kv8)
        runs = {"dense_observe_ms": base_obs, "observe_ms": obs, "dense_call_ms": base_call,
                "call_ms": call}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        times = {key: [] for key in runs}
        for _ in range(rounds):  # alternating
            for key, fn in runs.items():
                times[key].append(timed(fn, reps))
        rec = {"geometry": name, "source": src, "layers": L, "seq": S, "kv_heads": Hkv, "group": G,
               "window": W, "rounds": rounds, "lib": os.path.basename(N.LIB_PATH)}
        for key, v in times.items():
            rec[key] = round(statistics.median(v), 4)
            rec[key + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
        rec["observe_vs_dense"] = round(rec["observe_ms"] / rec["dense_observe_ms"], 3)
        rec["call_vs_dense"] = round(rec["call_ms"] / rec["dense_call_ms"], 3)
        lines.append(json.dumps(rec))
        del obs, call, runs
        torch.cuda.empty_cache()
    return lines


def wide(name, L, S, Hkv, G, rounds, reps, gen):
    """A wide query group (kvc_observe_wide.h): the observe set and the whole snapkv_compress call
    beside the two ways round it: the query heads split into observation_scores calls of groups
    the 4-block schedule admits at pooling_kernel = 1 (G = 8: two G = 4 calls; G = 7: G = 4, 2 and
    1), added and pooled in torch; and the torch line."""
    kv = [tuple(torch.empty(1, Hkv, S, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
                for _ in range(2)) for _ in range(L)]
    qs = [torch.empty(1, G * Hkv, W, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
          for _ in range(L)]
    ks = [k for k, _ in kv]
    jobs = [E.Segments(i, k, v, zone_len=S - W, n_select=KEEP - W, tail_start=S - W, tail_len=W)
            for i, (k, v) in enumerate(kv)]
    table = E._build_table(0, torch.bfloat16, 1, Hkv, D, jobs)
    obs = observe_set(torch.bfloat16, Hkv, G, table[0], qs)
    # the admitted groups the heads split into, as slices of a KV head's G query heads
    parts, g0 = [], 0
    for g in (4, 2, 1):
        while G - g0 >= g:
            parts.append((g0, g))
            g0 += g
    qparts = [[q.view(1, Hkv, G, W, D)[:, :, a:a + g].reshape(1, Hkv * g, W, D).contiguous()
               for q in qs] for a, g in parts]

    def split():
        out = None
        for qp in qparts:
            imp = torch.stack(observation_scores(ks, qp, pooling_kernel=1))
            out = imp if out is None else out + imp
        return F.avg_pool1d(out.flatten(0, 2)[None], POOL, 1, POOL // 2)

    runs = {"observe_ms": obs, "split_ms": split,
            "call_ms": lambda: snapkv_compress(kv, qs, W, KEEP, POOL),
            "torch_ms": lambda: torch_scores(kv, qs, G)}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    times = {key: [] for key in runs}
    for _ in range(rounds):  # alternating
        for key, fn in runs.items():
            times[key].append(timed(fn, reps if key != "torch_ms" else 2))
    rec = {"geometry": name, "layers": L, "seq": S, "kv_heads": Hkv, "group": G, "window": W,
           "split_groups": [g for _, g in parts], "k_bytes": L * Hkv * S * D * 2,
           "rounds": rounds, "lib": os.path.basename(N.LIB_PATH)}
    for key, v in times.items():
        rec[key] = round(statistics.median(v), 4)
        rec[key + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    rec["observe_vs_split"] = round(rec["observe_ms"] / rec["split_ms"], 3)
    rec["observe_gbps_two_reads"] = round(2 * rec["k_bytes"] / rec["observe_ms"] / 1e6, 1)
    return json.dumps(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--seq", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--sources", action="store_true",
                    help="paged (P = 16, 128) and fp8 keys next to the dense bf16 set")
    ap.add_argument("--wide", action="store_true",
                    help="wide query groups (G = 8 and G = 7 at W = 32) next to the split calls")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("observe_bench needs the GPU")
    gen = torch.Generator(device=DEV).manual_seed(0)
    geos = (("mha_h32", 32, 1), ("gqa_h8_g4", 8, 4))
    if a.wide:
        lines = [wide(n, a.layers, a.seq, h, g, a.rounds, a.reps, gen)
                 for n, h, g in (("gqa_h8_g8", 8, 8), ("gqa_h8_g7", 8, 7))]
    elif a.sources:
        lines = [ln for n, h, g in geos
                 for ln in sources(n, a.layers, a.seq, h, g, a.rounds, a.reps, gen)]
    else:
        lines = [json.dumps(geometry(n, a.layers, a.seq, h, g, a.rounds, a.reps, gen))
                 for n, h, g in geos]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
