"""Does a stream-capture query between launches cost GPU time?  (The engine asks
torch.cuda.is_current_stream_capturing() once per call: INTEGRATION.md, "CUDA graphs".)  The
headline step, timed in blocks of 20 steps, with 0 / 1 / 10 extra queries before every step,
alternating the variants block by block in one process; the query's host cost on an idle device.
GPU box only (evidence: profiles/r07_graph_capture_bench_more.jsonl)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs3602-llm-inference-acceleration_amd"))
from kvcompress.methods import get_compress_fn  # noqa: E402

dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1000)
layers = [(torch.randn(1, 32, 16384, 128, device=dev, generator=g).to(torch.bfloat16),
           torch.randn(1, 32, 16384, 128, device=dev, generator=g).to(torch.bfloat16))
          for _ in range(32)]
fn = get_compress_fn("fix_size_l2")
q = torch.cuda.is_current_stream_capturing


def block(extra, steps=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        for _ in range(extra):
            q()
        fn(layers, skip_layers=[], fix_kv_size=512, keep_ratio=0.0, strategy="keep_low")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


for _ in range(3):
    block(0)
res = {0: [], 1: [], 10: []}
for _ in range(25):
    for extra in (0, 1, 10):
        res[extra].append(block(extra))
out = {str(k): {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
       for k, v in res.items()}
torch.cuda.synchronize()
n = 200000
t0 = time.perf_counter()
for _ in range(n):
    q()
out["is_current_stream_capturing_us"] = (time.perf_counter() - t0) / n * 1e6
print(json.dumps(out))
