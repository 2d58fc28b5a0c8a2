"""What saying where the result goes is worth ("Destinations"): one compress call over
32 layers whose inputs are windows of a static cache, three ways --
  A  what a caller without destinations does: the default call, then
     window[:, :, :n].copy_(out) per tensor (64 copies);
  B  out="inplace";
  C  out=[...] into a second static cache.
The variants alternate in one process; each sample is `reps` calls between two device events
(after warm-up), reported per call.  A library without the destination entries (the parent
commit's, built by tools/build_variant.sh and selected with KVC_LIB) runs variant A alone.
Every call compacts what the previous one left in the cache -- the same for all variants.
One JSON line per (shape, variant).  GPU box only.

  python tools/dest_bench.py [--shapes headline,l2,streaming,decode] [--rounds 5] [--tag NAME]
                             [--variants A,B,C] [--layers 32]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs3602-llm-inference-acceleration_amd"))
from kvcompress import _native as N  # noqa: E402
from kvcompress.methods import get_compress_fn  # noqa: E402

DEV = torch.device("cuda:0")
L, H, D, PAD = 32, 32, 128, 37
SHAPES = {
    "headline": ("fix_size_l2", dict(fix_kv_size=512, keep_ratio=0.0, skip_layers=[]), 16384),
    "l2": ("l2_compress", dict(keep_ratio=0.8, skip_layers=[]), 16384),
    "streaming": ("streaming_llm", dict(start_size=4, recent_size=508, skip_layers=[]), 16384),
    "decode": ("fix_size_l2", dict(fix_kv_size=512, keep_ratio=0.0, skip_layers=[]), 513),
}


def caches(S, gen):
    out = []
    for _ in range(L):
        kv = []
        for _ in range(2):
            c = torch.empty(1, H, S + PAD, D, dtype=torch.bfloat16, device=DEV)
            c.normal_(generator=gen)
            kv.append(c)
        out.append(tuple(kv))
    return out


def sample(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,l2,streaming,decode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--variants", default="A,B,C", help="subset of A,B,C (e.g. B under rocprofv3)")
    ap.add_argument("--layers", type=int, default=32,
                    help="layers per call (4: fewer (layer, head) rows than CUs)")
    args = ap.parse_args()
    global L
    L = args.layers
    has_dest = hasattr(N.lib(), "kvc_plan_dest")
    gen = torch.Generator(device=DEV).manual_seed(0)
    for name in args.shapes.split(","):
        method, kw, S = SHAPES[name]
        fn = get_compress_fn(method)
        src = caches(S, gen)
        win = [(k[:, :, :S], v[:, :, :S]) for k, v in src]

        def run_a():
            out = fn(list(win), **kw)
            for (k, v), (ko, vo) in zip(win, out):
                k[:, :, :ko.shape[2]].copy_(ko)
                v[:, :, :vo.shape[2]].copy_(vo)

        variants = {"A": run_a}
        n_out = fn(list(win), **kw)[0][0].shape[2]
        if has_dest:
            dst = caches(n_out, gen)  # a second cache, S_max = n_out + PAD
            variants["B"] = lambda: fn(list(win), out="inplace", **kw)
            variants["C"] = lambda: fn(list(win), out=list(dst), **kw)
        variants = {v: f for v, f in variants.items() if v in args.variants.split(",")}
        # one call of the long shapes moves GBs: a few calls per sample are well above 1 ms;
        # the decode step takes ~0.1 ms
        reps = 40 if S < 4096 else 4
        for f in variants.values():  # warm-up: plan caches, call memo, allocator
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v, f in variants.items():
                times[v].append(sample(f, reps))
        for v, ts in times.items():
            print(json.dumps(dict(tool="dest_bench", tag=args.tag, shape=name, method=method, S=S,
                                  layers=L, n_out=n_out, variant=v, lib=os.path.basename(N.LIB_PATH),
                                  ms_median=round(statistics.median(ts), 4),
                                  ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                                  reps=reps, rounds=args.rounds)), flush=True)
        del src, win, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
