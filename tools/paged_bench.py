"""What reading K / V through a block table costs ("Paged caches"): one in-place
compress call over 32 layers of [1, 32, S, 128] bf16, fix_size_l2(512) --
  dense   out="inplace" on windows of dense static caches (the baseline);
  paged   compress_paged in place on page pools with SHUFFLED block tables, pages of 16 and of
          128 tokens, pools stored [N, H, P, D] ("nhpd") and [N, P, H, D] ("nphd", vLLM's).
The variants alternate in one process.  Per variant: the call's device time (`reps` calls between
two device events, per call), SCORE / SELECT / GATHER separately (the engine's phase timer: three
launches, fenceless events), and the host time one call takes to enqueue (`host_us`: what a
native replay of paged decode steps would have to beat).  Every call compacts what the previous
one left in the cache -- the same for all variants.  One JSON line per (shape, variant); the
comparison to watch is paged SCORE over dense SCORE at P = 128, nhpd (`score_vs_dense`).
GPU box only.

  python tools/paged_bench.py [--shapes headline,decode] [--rounds 5] [--layers 32] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs3602-llm-inference-acceleration_amd"))
from kvcompress import PagedKV, compress_paged  # noqa: E402
from kvcompress import _engine as E  # noqa: E402
from kvcompress.methods import get_compress_fn  # noqa: E402

DEV = torch.device("cuda:0")
H, D, PAD, SPARE = 32, 128, 37, 7
METHOD, KW = "fix_size_l2", dict(fix_kv_size=512, keep_ratio=0.0, skip_layers=[])
SHAPES = {"headline": 16384, "decode": 513}
PAGED = [(P, st) for P in (16, 128) for st in ("nhpd", "nphd")]


def dense_layers(L, S, gen):
    out = []
    for _ in range(L):
        kv = [torch.empty(1, H, S + PAD, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
              for _ in range(2)]
        out.append((kv[0][:, :, :S], kv[1][:, :, :S]))
    return out


def paged_layers(L, S, P, storage, gen):
    npp = -(-S // P)
    n = npp + SPARE
    out = []
    for _ in range(L):
        pools = []
        for _ in range(2):
            shape = (n, H, P, D) if storage == "nhpd" else (n, P, H, D)
            back = torch.empty(shape, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
            pools.append(back if storage == "nhpd" else back.permute(0, 2, 1, 3))
        table = torch.randperm(n, generator=gen, device=DEV)[:npp].to(torch.int32).reshape(1, npp)
        out.append(PagedKV(pools[0], pools[1], table, S))
    return out


def sample(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def phases(fn, reps):
    """Median SCORE / SELECT / GATHER ms of `reps` calls launched phase by phase."""
    t = E.PhaseTimer(split=True, steps=E.PhaseTimer.THREE, fenceless=True)
    E.set_phase_timer(t)
    try:
        for _ in range(reps):
            fn()
        d = t.durations_ms()
    finally:
        E.set_phase_timer(None)
    return {k: round(statistics.median(v), 4) for k, v in d.items()}


def host_us(fn, reps):
    """Host time to enqueue one call (the device idle at the start, not waited for in between)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return round(dt / reps * 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,decode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    L = args.layers
    gen = torch.Generator(device=DEV).manual_seed(0)
    dense_fn = get_compress_fn(METHOD)
    lines = []
    for name in args.shapes.split(","):
        S = SHAPES[name]
        reps = 40 if S < 4096 else 4
        dense = dense_layers(L, S, gen)
        variants = {("dense", 0, "bhsd"): lambda: dense_fn(list(dense), out="inplace", **KW)}
        keep = [dense]
        for P, st in PAGED:
            layers = paged_layers(L, S, P, st, gen)
            keep.append(layers)
            variants[("paged", P, st)] = lambda layers=layers: compress_paged(METHOD, layers, **KW)
        for f in variants.values():  # warm-up
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v, f in variants.items():
                times[v].append(sample(f, reps))
        ph = {v: phases(f, max(reps, 8)) for v, f in variants.items()}
        host = {v: host_us(f, max(reps, 8)) for v, f in variants.items()}
        base = ph[("dense", 0, "bhsd")]
        for v, ts in times.items():
            lines.append(dict(
                tool="paged_bench", shape=name, method=METHOD, S=S, layers=L, variant=v[0],
                page_size=v[1], storage=v[2], ms_median=round(statistics.median(ts), 4),
                ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), ms_score=ph[v].get("score"),
                ms_select=ph[v].get("select"), ms_gather=ph[v].get("gather"),
                score_vs_dense=round(ph[v]["score"] / base["score"], 3),
                gather_vs_dense=round(ph[v]["gather"] / base["gather"], 3),
                host_us=host[v], reps=reps, rounds=args.rounds))
            print(json.dumps(lines[-1]), flush=True)
        del dense, variants, keep
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
