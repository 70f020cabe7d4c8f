#!/usr/bin/env python3
"""Times of attention_tiled_kernel (csrc/attention_tiled.h) for profiles/attention_tiled.txt:

  1. the kernel alone at (B, H, T) = (64, 16, 577) and (8, 16, 577), bf16 and MXFP8 output: us per launch, TFLOP/s (4 T^2 64 per pair);
  2. against attention_long_kernel where both run, (8, 16, 257) and (8, 16, 288), through mmiss_dbg_attention_tiled and
     mmiss_dbg_attention (128 pairs: below the streaming kernel's threshold) — the price of chunking;
  3. images/s of a 24-layer ViT-L/14@336 encode at batch 64 under "bf16" and "fp8" (seeded random weights).

HIP events around single launches, the candidates of a comparison interleaved round by round in one process; median and
minimum over the rounds; Gaussian data (zero operands read high). Usage: python tools/attention_tiled_time.py [rounds] [--no-encode]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import mmiss_amd  # noqa: F401
from mmiss_amd import _lib
from mmiss_amd.encoder import VIT_L14_336, ClipEncoder, random_state_dict

lib = _lib.load()
ROUNDS = int(next((a for a in sys.argv[1:] if a.isdigit()), 30))


def interleaved(cands, rounds=ROUNDS, warmup=3):
    """cands: {name: callable launching once on the null stream} -> {name: (median us, min us)}."""
    times = {k: [] for k in cands}
    for r in range(warmup + rounds):
        for k, fn in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[k].append(a.elapsed_time(b) * 1e3)
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}


def buffers(B, T, H):
    d = H * 64
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + T)
    qkv = torch.randn(B * T, 3 * d, device="cuda", generator=g).to(torch.bfloat16)
    ctx = torch.empty(B * T, d, device="cuda", dtype=torch.bfloat16)
    c8 = torch.empty(B * T, d, device="cuda", dtype=torch.uint8)
    cs = torch.empty(B * T, 16 * ((d + 511) // 512), device="cuda", dtype=torch.uint8)
    return qkv, ctx, c8, cs


def tiled(qkv, ctx, B, T, H):
    return lambda: _lib.check(lib.mmiss_dbg_attention_tiled(0, None, qkv.data_ptr(), ctx.data_ptr(), None, None, B, T, H, 0))


def tiled_mx(qkv, c8, cs, B, T, H):
    return lambda: _lib.check(lib.mmiss_dbg_attention_tiled(0, None, qkv.data_ptr(), None, c8.data_ptr(), cs.data_ptr(), B, T, H, 0))


print(f"rounds = {ROUNDS}, one launch per event pair, interleaved")
for B, H, T in ((64, 16, 577), (8, 16, 577)):
    qkv, ctx, c8, cs = buffers(B, T, H)
    res = interleaved({"bf16 out": tiled(qkv, ctx, B, T, H), "MXFP8 out": tiled_mx(qkv, c8, cs, B, T, H)})
    for k, (med, mn) in res.items():
        print(f"tiled  B={B:3d} H={H} T={T}  {k:9s}  median {med:8.1f} us  min {mn:8.1f} us  {4.0 * B * H * T * T * 64 / med / 1e6:6.1f} TFLOP/s (median)")

for B, H, T in ((8, 16, 257), (8, 16, 288)):
    qkv, ctx, c8, cs = buffers(B, T, H)
    ctx2 = torch.empty_like(ctx)
    long_ = lambda: _lib.check(lib.mmiss_dbg_attention(0, None, qkv.data_ptr(), ctx2.data_ptr(), B, T, H, 0))
    res = interleaved({"attention_long_kernel": long_, "attention_tiled_kernel": tiled(qkv, ctx, B, T, H)})
    torch.cuda.synchronize()
    for k, (med, mn) in res.items():
        print(f"both   B={B:3d} H={H} T={T}  {k:22s}  median {med:8.1f} us  min {mn:8.1f} us")
    print(f"       tiled / long (median) = {res['attention_tiled_kernel'][0] / res['attention_long_kernel'][0]:.3f}, equal bits: {bool(torch.equal(ctx, ctx2))}")

if "--no-encode" not in sys.argv:
    B = 64
    W = random_state_dict(VIT_L14_336, 0)
    px = torch.from_numpy(np.random.Generator(np.random.Philox(1)).standard_normal((B, 3, 336, 336), dtype=np.float32)).cuda()
    enc = ClipEncoder(VIT_L14_336, max_batch_image=B, max_batch_text=1)
    enc.load_state_dict(W)
    del W
    for prec in ("bf16", "fp8"):
        enc.set_precision(prec)
        res = interleaved({prec: lambda: enc.encode_image(px)}, rounds=max(5, ROUNDS // 3), warmup=2)
        med, mn = res[prec]
        print(f"encode ViT-L/14@336, 24 layers, batch {B}, {prec:4s}: median {med / 1e3:7.2f} ms = {B / med * 1e6:7.0f} images/s (best {B / mn * 1e6:7.0f})")
    enc.close()
