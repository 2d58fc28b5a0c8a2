"""What an fp8 KV cache costs to compress, against bf16 in the same process on the same box
("fp8 caches"): the headline geometry -- fix_size_l2(512) over 32 layers of
[1, 32, 16384, 128] -- with K/V stored as float8_e4m3fn, float8_e5m2 and bfloat16.

Per dtype, alternating between them in every round:
  plain   the default call: device time of `reps` calls between two device events, per call;
  phases  SCORE and SELECT_GATHER launched and timed separately (the engine's phase timer,
          fenceless events): median kernel time of each;
  paged   compress_paged in place on [N, P, H, D] pools of 16-token pages behind a shuffled block
          table: device time per call and its SCORE / SELECT / GATHER kernels.
SCORE reads every zone key once and writes a 2-byte norm per token: `score_bytes` is computed from
the shapes, `score_gbps` is that over the measured SCORE time, and `score_rate_vs_bf16` the
fraction of the bf16 SCORE kernel's bytes/s the fp8 kernel achieves (1.0 = as HBM-bound as bf16;
`score_time_vs_bf16` is the plain time ratio, 0.5 at best).  One JSON line per (variant, dtype).
GPU box only; every call compresses fresh copies' worth of data already resident (the dense calls
do not modify their inputs; the paged calls compact what the previous one left, the same for all
dtypes).

  python tools/fp8_bench.py [--rounds 7] [--reps 64] [--layers 32] [--S 16384] [--out FILE]

The counters quoted in DESIGN.md come from a run of this tool under the profiler, on its own and
without tracing; tools/fp8_pmc_summary.py records the command and aggregates its output.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs3602-llm-inference-acceleration_amd"))
from kvcompress import PagedKV, compress_paged  # noqa: E402
from kvcompress import _engine as E  # noqa: E402
from kvcompress.methods import get_compress_fn  # noqa: E402

DEV = torch.device("cuda:0")
H, D, P, SPARE = 32, 128, 16, 7
METHOD, KW = "fix_size_l2", dict(fix_kv_size=512, keep_ratio=0.0, skip_layers=[])
DTYPES = (("bf16", torch.bfloat16), ("e4m3", torch.float8_e4m3fn), ("e5m2", torch.float8_e5m2))


def normal(shape, dtype, gen):
    """N(0, 1) values rounded to `dtype` (fp8: through bfloat16, as a quantising cache would)."""
    x = torch.empty(shape, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
    return x if dtype is torch.bfloat16 else x.to(dtype)


def dense_layers(L, S, dtype, gen):
    return [(normal((1, H, S, D), dtype, gen), normal((1, H, S, D), dtype, gen))
            for _ in range(L)]


def paged_layers(L, S, dtype, gen):
    npp = -(-S // P)
    n = npp + SPARE
    out = []
    for _ in range(L):
        pools = [normal((n, P, H, D), dtype, gen).permute(0, 2, 1, 3) for _ in range(2)]
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


def phases(fn, reps, steps):
    t = E.PhaseTimer(split=True, steps=steps, fenceless=True)
    E.set_phase_timer(t)
    try:
        for _ in range(reps):
            fn()
        d = t.durations_ms()
    finally:
        E.set_phase_timer(None)
    return {k: round(statistics.median(v), 4) for k, v in d.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--S", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=64,
                    help="calls per timed window (64 calls: 30 - 70 ms of device time)")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fp8_bench needs the GPU"
    L, S, reps = args.layers, args.S, args.reps
    gen = torch.Generator(device=DEV).manual_seed(0)
    fn = get_compress_fn(METHOD)
    E.call_memo.clear()
    variants, keep = {}, []
    for name, dtype in DTYPES:
        dense = dense_layers(L, S, dtype, gen)
        paged = paged_layers(L, S, dtype, gen)
        keep += [dense, paged]
        variants[("plain", name)] = lambda dense=dense: fn(list(dense), **KW)
        variants[("paged", name)] = lambda paged=paged: compress_paged(METHOD, paged, **KW)
    for f in variants.values():  # warm-up: code objects, plan cache, native replay
        for _ in range(4):
            f()
    torch.cuda.synchronize()
    times = {v: [] for v in variants}
    for _ in range(args.rounds):  # the dtypes alternate inside every round
        for v, f in variants.items():
            times[v].append(sample(f, reps))
    ph = {}
    for v, f in variants.items():
        steps = E.PhaseTimer.DEFAULT if v[0] == "plain" else E.PhaseTimer.THREE
        ph[v] = phases(f, max(32, reps), steps)
    esz = {"bf16": 2, "e4m3": 1, "e5m2": 1}
    zone = S  # fix_size_l2(512, keep_ratio 0): every token is scored
    lines = []
    for v, ts in times.items():
        kind, name = v
        score_bytes = L * H * zone * (D * esz[name] + 2)  # keys read + bf16 norms written
        base = ph[(kind, "bf16")]
        base_bytes = L * H * zone * (D * 2 + 2)
        rate = score_bytes / ph[v]["score"]
        base_rate = base_bytes / base["score"]
        line = dict(tool="fp8_bench", variant=kind, dtype=name, method=METHOD, S=S, layers=L, H=H,
                    D=D, page_size=P if kind == "paged" else 0,
                    ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4),
                    ms_max=round(max(ts), 4), ms_score=ph[v]["score"],
                    score_bytes=score_bytes, score_gbps=round(rate / 1e6, 1),
                    score_time_vs_bf16=round(ph[v]["score"] / base["score"], 3),
                    score_rate_vs_bf16=round(rate / base_rate, 3), reps=reps, rounds=args.rounds)
        for k in ("select+gather", "select", "gather"):
            if k in ph[v]:
                line["ms_" + k.replace("+", "_")] = ph[v][k]
                line[k.replace("+", "_") + "_vs_bf16"] = round(ph[v][k] / base[k], 3)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
