"""What per-token scales cost an fp8 paged cache, against the SAME cache without them in the same
process on the same box ("fp8 caches", Scaled): the headline geometry as a paged cache
-- fix_size_l2(512) over 32 layers of [1, 32, 16384, 128], pages of 16 tokens stored [N, P, H, D]
behind a shuffled block table -- as float8_e4m3fn and float8_e5m2, with float32 K and V scale
pools stored [N, P, H] or [N, H, P] (kvc_launch_scaled) and without (kvc_launch_paged: the
yardstick, never the scaled run itself).

Per (dtype, unscaled / scale storage), the six variants alternating inside every round:
  call    device time of `reps` compress_paged calls between two device events, per call;
  phases  SCORE, SELECT and GATHER launched and timed separately (the engine's phase timer,
          fenceless events): the median kernel time of each window of `reps` calls.
Both are reported as the median over the rounds with min and max.  From the bytes alone SCORE
reads 4 more bytes per 128-byte key row and GATHER moves 8 more bytes per 256 bytes of a kept row
pair, about 3 % each; `*_vs_unscaled` is the ratio of medians.  One JSON line per variant.
GPU box only.  (Every call compacts what the previous one left: the same work for all variants.)

  python tools/scaled_bench.py [--rounds 7] [--reps 64] [--layers 32] [--S 16384] [--out FILE]
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

DEV = torch.device("cuda:0")
H, D, P, SPARE = 32, 128, 16, 7
METHOD, KW = "fix_size_l2", dict(fix_kv_size=512, keep_ratio=0.0, skip_layers=[])
DTYPES = (("e4m3", torch.float8_e4m3fn, 448.0), ("e5m2", torch.float8_e5m2, 57344.0))


def layers(L, S, dtype, amax, gen, scaled):
    """Per-token quantised pools: rows of N(0, 1) times a per-row magnitude in 2^-3 .. 2^3, each
    divided by its own scale amax(row) / amax(format); the scales in pools stored [N, P, H]
    (scaled == "nph": the heads' scales of a token share a cache line) or [N, H, P] ("nhp": a
    head's scales of a page are contiguous); False: no scales."""
    npp = -(-S // P)
    n = npp + SPARE
    out = []
    for _ in range(L):
        pools, scales = [], []
        for _ in range(2):
            x = torch.empty((n, P, H, D), dtype=torch.float32, device=DEV).normal_(generator=gen)
            x *= torch.exp2(torch.empty((n, P, H, 1), device=DEV).uniform_(-3, 3, generator=gen))
            s = x.abs().amax(dim=-1) / amax
            pools.append((x / s[..., None]).to(dtype).permute(0, 2, 1, 3))
            s = s.permute(0, 2, 1)
            scales.append(s.contiguous() if scaled == "nhp" else s)
        table = torch.randperm(n, generator=gen, device=DEV)[:npp].to(torch.int32).reshape(1, npp)
        kw = dict(k_scale=scales[0], v_scale=scales[1]) if scaled else {}
        out.append(PagedKV(pools[0], pools[1], table, S, **kw))
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
    t = E.PhaseTimer(split=True, steps=E.PhaseTimer.THREE, fenceless=True)
    E.set_phase_timer(t)
    try:
        for _ in range(reps):
            fn()
        d = t.durations_ms()
    finally:
        E.set_phase_timer(None)
    return {k: statistics.median(v) for k, v in d.items()}


def stats(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4),
                max=round(max(xs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--S", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=64)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scaled_bench needs the GPU"
    L, S, reps = args.layers, args.S, args.reps
    gen = torch.Generator(device=DEV).manual_seed(0)
    variants = {}
    for name, dtype, amax in DTYPES:
        for scaled in (False, "nph", "nhp"):
            pk = layers(L, S, dtype, amax, gen, scaled)
            variants[(name, scaled)] = lambda pk=pk: compress_paged(METHOD, pk, **KW)
    for f in variants.values():
        for _ in range(4):
            f()
    torch.cuda.synchronize()
    calls = {v: [] for v in variants}
    ph = {v: {} for v in variants}
    for _ in range(args.rounds):  # scaled and unscaled alternate inside every round
        for v, f in variants.items():
            calls[v].append(sample(f, reps))
        for v, f in variants.items():
            for k, x in phases(f, max(32, reps)).items():
                ph[v].setdefault(k, []).append(x)
    lines = []
    for (name, scaled), ts in calls.items():
        base = (name, False)
        line = dict(tool="scaled_bench", dtype=name, scaled=scaled, method=METHOD, S=S, layers=L,
                    H=H, D=D, page_size=P, reps=reps, rounds=args.rounds, ms_call=stats(ts),
                    call_vs_unscaled=round(statistics.median(ts) /
                                           statistics.median(calls[base]), 3))
        for k, xs in ph[(name, scaled)].items():
            line["ms_" + k] = stats(xs)
            line[k + "_vs_unscaled"] = round(statistics.median(xs) /
                                             statistics.median(ph[base][k]), 3)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
