#!/usr/bin/env python3
"""Wall time of one ClipEncoder.calibrate call on ViT-B/32 (HIP events on the call's stream, device pixels, median of 5) at
B = 64 and B = 256, and the kernels it launches. No bar is attached: calibration is one-shot (profiles/fp8_calibration.txt)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import mmiss_amd  # noqa: F401
from mmiss_amd import _lib
from mmiss_amd.encoder import ClipEncoder, VIT_B32, random_state_dict


def main():
    W = random_state_dict(VIT_B32, seed=0)
    enc = ClipEncoder(VIT_B32, max_batch_image=256, max_batch_text=8, precision="fp8")
    enc.load_state_dict(W)
    for B in (64, 256):
        px = torch.randn((B, 3, 224, 224), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
        enc.calibrate(px)   # warm-up: workspaces, code objects
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            info = enc.calibrate(px)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        _lib.prof_filter(None, 1)
        _lib.prof_reset()
        _lib.prof_enable(True)
        enc.calibrate(px)
        _lib.prof_enable(False)
        kern = {p["kernel"]: (p["launches"], round(p["ms"], 3)) for p in _lib.prof_read()
                if p["kernel"] in ("ln_colstats", "colstats_finish", "bias_fold")}
        print(f"calibrate B={B} ({info['rows']} rows, {info['centred']} channels centred): median {np.median(ms):.2f} ms "
              f"(5 calls: {' '.join('%.2f' % m for m in ms)}); new kernels (launches, total ms): {kern}", flush=True)
    enc.close()


if __name__ == "__main__":
    main()
