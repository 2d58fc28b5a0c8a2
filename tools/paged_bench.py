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

--ragged measures batches with a length per sequence (kvc_launch_ragged) instead, P = 16, nhpd:
  a_batch_vs_loop   B = 8 and 64 sequences of 600..16 384 rows: one ragged call against the loop
                    of B single-sequence calls, host and GPU time separately;
  b_envelope        a 16 384-row sequence beside seven of 600, alone, and the seven alone: what
                    the short rows pay for the long row's grid and kernel class;
  c_uniform         the headline call as a list of equal lengths (ragged kernels) and as an int
                    (the existing kernels): the price of the record indirection;
  d_host_planning   host planning time against the number of distinct length profiles.
--repage measures paged DESTINATIONS (kvc_launch_repage; DESIGN.md, "Paged destinations"), P = 16,
pools stored [N, P, H, D], in three alternating rounds of all four configurations (one JSON line
per round and configuration, so the spread is visible):
  a_inplace          the headline call compacted in place (the existing kernels);
  b_fresh_pages      the same call into fresh pages of the same pool (out=[PagedDest(table)]);
  c_ragged_inplace / c_ragged_fresh   the ragged profile of --ragged (B = 8, lengths 600 .. 16 384,
                     8 heads), in place against into fresh pages.
The figure to watch is `gpu_ms_gather` of b against a (and of c_ragged_fresh against
c_ragged_inplace): the out-of-place copy moves the same bytes plus the sink rows, with its passes
side by side instead of one workgroup per row.
`ms_call` is event to event around whole calls (host-bound when the GPU is idle between
launches), `gpu_ms*` the summed kernel durations of a call's launches, `host_us` the enqueue time.
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


# ---- --ragged: per-sequence lengths in one launch set ("Ragged paged batches") --------
def ragged_pools(L, lens, heads, P, gen):
    """L layers of one nhpd pool pair holding len(lens) sequences behind a shuffled [B, pages]
    table (entries past a sequence's last page are 0: valid, never read)."""
    npp = [-(-n // P) for n in lens]
    n = sum(npp) + SPARE
    out = []
    for _ in range(L):
        pools = [torch.empty(n, heads, P, D, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
                 for _ in range(2)]
        perm = torch.randperm(n, generator=gen, device=DEV).to(torch.int32)
        table = torch.zeros(len(lens), max(npp), dtype=torch.int32, device=DEV)
        at = 0
        for b, c in enumerate(npp):
            table[b, :c] = perm[at:at + c]
            at += c
        out.append((pools[0], pools[1], table))
    return out


def gpu_ms(fn, reps):
    """Kernel time of one call: the SCORE / SELECT / GATHER durations of all its launches, summed
    (fenceless events around every launch), per call."""
    t = E.PhaseTimer(split=True, steps=E.PhaseTimer.THREE, fenceless=True)
    E.set_phase_timer(t)
    try:
        for _ in range(reps):
            fn()
        d = t.durations_ms()
    finally:
        E.set_phase_timer(None)
    return {k: round(sum(v) / reps, 4) for k, v in d.items()}


def measure(fn, reps, rounds):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = [sample(fn, reps) for _ in range(rounds)]
    g = gpu_ms(fn, reps)
    return dict(ms_call_median=round(statistics.median(ts), 4), ms_call_min=round(min(ts), 4),
                ms_call_max=round(max(ts), 4), gpu_ms_score=g.get("score", 0.0),
                gpu_ms_select=g.get("select", 0.0), gpu_ms_gather=g.get("gather", 0.0),
                gpu_ms=round(sum(g.values()), 4), host_us=host_us(fn, reps), reps=reps,
                rounds=rounds)


def spread(B, lo=600, hi=16384):
    """B lengths from lo to hi, geometrically spaced (many short sequences, few long ones)."""
    if B == 1:
        return [hi]
    return [int(round(lo * (hi / lo) ** (i / (B - 1)))) for i in range(B)]


def ragged_main(args):
    from kvcompress import paged as PG
    L, P, gen = args.layers, 16, torch.Generator(device=DEV).manual_seed(0)
    lines = []

    def emit(**kw):
        lines.append(dict(tool="paged_bench", mode="ragged", method=METHOD, layers=L, page_size=P,
                          dtype="bf16", D=D, **kw))
        print(json.dumps(lines[-1]), flush=True)

    def calls(pools, rows, lens):
        """(the ragged call, the loop of single-sequence calls) over table rows `rows`."""
        rag = [PagedKV(k, v, t[rows], [lens[b] for b in rows]) for k, v, t in pools]
        one = [[PagedKV(k, v, t[b:b + 1], lens[b]) for k, v, t in pools] for b in rows]
        return (lambda: compress_paged(METHOD, rag, **KW),
                lambda: [compress_paged(METHOD, x, **KW) for x in one])

    # (a) a batch against the loop of single-sequence calls (the only thing a PagedKV with one
    # int length can run); heads = 8 keeps the 64-sequence pools near 40 GiB
    heads = 8
    lens = spread(64)
    pools = ragged_pools(L, lens, heads, P, gen)
    for B in (8, 64):
        rows = list(range(0, 64, 64 // B))
        rag, loop = calls(pools, rows, lens)
        for name, fn in (("ragged", rag), ("loop", loop)):
            emit(part="a_batch_vs_loop", B=B, H=heads, variant=name, tokens=sum(lens[b] for b in rows),
                 **measure(fn, 2 if B == 64 else 4, args.rounds))
    del pools
    torch.cuda.empty_cache()
    # (b) what the envelope costs: one long sequence beside seven short ones
    lens = [16384] + [600] * 7
    pools = ragged_pools(L, lens, heads, P, gen)
    for name, rows in (("A_long_and_seven_short", list(range(8))), ("B_long_alone", [0]),
                       ("C_seven_short", list(range(1, 8)))):
        rag, _ = calls(pools, rows, lens)
        emit(part="b_envelope", batch=name, B=len(rows), H=heads, **measure(rag, 8, args.rounds))
    del pools
    torch.cuda.empty_cache()
    # (c) uniform lengths at the paged headline geometry: the list runs the ragged kernels, the
    # int the existing ones -- the price of the record indirection
    pools = ragged_pools(L, [16384], H, P, gen)
    for name, fn in (("list_of_equal_lengths", calls(pools, [0], [16384])[0]),
                     ("int", lambda: compress_paged(
                         METHOD, [PagedKV(k, v, t, 16384) for k, v, t in pools], **KW))):
        emit(part="c_uniform", B=1, H=H, S=16384, variant=name, **measure(fn, 4, args.rounds))
    del pools
    torch.cuda.empty_cache()
    # (d) host planning time against the number of distinct length profiles (no GPU work)
    fn = get_compress_fn(METHOD)
    geo = [(heads, D, torch.bfloat16, DEV)] * L
    for distinct in (1, 8, 64):
        base = spread(distinct)
        lens = [base[b % distinct] for b in range(64)]
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            PG.plan_ragged(fn, [lens] * L, geo, KW)
            ts.append((time.perf_counter() - t0) * 1e6)
        emit(part="d_host_planning", B=64, distinct_profiles=distinct,
             plan_us_median=round(statistics.median(ts), 1), plan_us_min=round(min(ts), 1))
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


# ---- --repage: pages to pages ("Paged destinations") ---------------------------------
def repage_main(args):
    from kvcompress import PagedDest
    L, P, gen = args.layers, 16, torch.Generator(device=DEV).manual_seed(0)
    keep = KW["fix_kv_size"]
    lines = []

    def pools(lens, heads):
        """L layers: nphd pool pair with room for the sources, `keep` fresh rows per sequence and
        the spare pages; the source table and the table of the fresh pages."""
        npp = [-(-n // P) for n in lens]
        fresh = -(-keep // P)
        n = sum(npp) + len(lens) * fresh + SPARE
        out = []
        for _ in range(L):
            kv = [torch.empty(n, P, heads, D, dtype=torch.bfloat16, device=DEV)
                  .normal_(generator=gen).permute(0, 2, 1, 3) for _ in range(2)]
            perm = torch.randperm(n, generator=gen, device=DEV).to(torch.int32)
            src = torch.zeros(len(lens), max(npp), dtype=torch.int32, device=DEV)
            at = 0
            for b, c in enumerate(npp):
                src[b, :c] = perm[at:at + c]
                at += c
            dst = perm[at:at + len(lens) * fresh].reshape(len(lens), fresh).contiguous()
            out.append((kv[0], kv[1], src, dst))
        return out

    configs, hold = {}, []
    for name, lens, heads, ragged in (("headline", [SHAPES["headline"]], H, False),
                                      ("ragged", spread(8), 8, True)):
        for fresh in (False, True):
            ps = pools(lens, heads)  # a pool set per configuration: in place rewrites its own
            hold.append(ps)
            layers = [PagedKV(k, v, t, list(lens) if ragged else lens[0]) for k, v, t, _ in ps]
            out = [PagedDest(d) for _, _, _, d in ps] if fresh else "inplace"
            key = ("c_ragged_" + ("fresh" if fresh else "inplace")) if ragged else \
                ("b_fresh_pages" if fresh else "a_inplace")
            configs[key] = (lambda layers=layers, out=out: compress_paged(METHOD, layers, out=out,
                                                                          **KW),
                            dict(B=len(lens), H=heads, tokens=sum(lens)))
    for fn, _ in configs.values():  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = 4
    for rnd in range(3):
        for key in sorted(configs):
            fn, info = configs[key]
            ms = sample(fn, reps)
            g = gpu_ms(fn, reps)
            lines.append(dict(tool="paged_bench", mode="repage", method=METHOD, layers=L,
                              page_size=P, storage="nphd", dtype="bf16", D=D, config=key,
                              round=rnd, ms_call=round(ms, 4), gpu_ms_score=g.get("score", 0.0),
                              gpu_ms_select=g.get("select", 0.0),
                              gpu_ms_gather=g.get("gather", 0.0), reps=reps, **info))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,decode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--ragged", action="store_true",
                    help="measure ragged batches (per-sequence lengths) instead of the shapes")
    ap.add_argument("--repage", action="store_true",
                    help="measure paged destinations (pages to pages) against in place")
    args = ap.parse_args()
    if args.ragged:
        return ragged_main(args)
    if args.repage:
        return repage_main(args)
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
