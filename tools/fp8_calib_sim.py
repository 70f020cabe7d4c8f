#!/usr/bin/env python3
"""CPU emulation (torch, fp32 arithmetic on dequantised values) of the ViT-B/32 vision tower under set_precision("fp8"), with
and without calibrated activation centring (mmiss_encoder_calibrate, DESIGN.md 3b "Outlier channels"):

    LN(x) W^T + b  =  (LN(x) - mu) W^T + (b + W mu)

mu = the per-channel mean of a LayerNorm output over a calibration batch (one bf16 pass over OTHER images); LN(x) - mu is
quantised to MXFP8, b + W mu is an f32 vector from the bf16 weights. Three forms per weight set:
  today    LayerNorm output -> MXFP8 as it is
  every    every channel centred
  rule     a channel centred only where mean^2 >= variance over the calibration rows (what the library builds)
on three weight sets: seeded Gaussian, +300 / -180 residual channels on every token row, the same on the CLS row only.
Prints 1 - cos of the embeddings against the fp32 tower. The helpers are this tool's own copy of tools/fp8_fold_sim.py's."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from oracle import clip_oracle as co

torch.set_num_threads(8)

CASES = (("no outliers", None), ("+300 / -180 on every token row", "all"), ("+300 / -180 on the CLS row only", "cls"))


def bf16(x):
    return x.to(torch.bfloat16).float()


def mx_quant(x):
    """rows x K -> dequantised MXFP8 (one E8M0 scale per 32 columns, e4m3 codes): gemm_fp8.h mx_scale_of"""
    r, k = x.shape
    b = x.reshape(r, k // 32, 32)
    amax = b.abs().amax(dim=-1, keepdim=True).clamp_min(1e-30) / 448.0
    e = torch.ceil(torch.log2(amax)).clamp(-126, 127)
    s = torch.exp2(e)
    q = (b / s).to(torch.float8_e4m3fn).float()
    return (q * s).reshape(r, k)


def w_quant(w):
    """[N, K] -> dequantised e4m3 with one f32 scale per output channel"""
    s = w.abs().amax(dim=1, keepdim=True).clamp_min(1e-30) / 448.0
    return (w / s).to(torch.float8_e4m3fn).float() * s


def ln_stats(x, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def tower(px, W, s, mode, table=None, device="cpu"):
    """mode "fp32": the reference arithmetic; "fp8": today's form; "collect": the bf16 pass, `table` (a list) receives one
    float64 (mean, variance) pair per LayerNorm site; "centred": fp8 with `table` = one mu vector per site."""
    T = lambda k: torch.from_numpy(W[k]).to(device)
    B = px.shape[0]
    pw = T("vision_model.embeddings.patch_embedding.weight").reshape(s.v_hidden, -1)
    patches = torch.from_numpy(co.patchify(px, s.v_patch)).to(device) @ pw.T
    cls = T("vision_model.embeddings.class_embedding").expand(B, 1, s.v_hidden)
    x = torch.cat([cls, patches], dim=1) + T("vision_model.embeddings.position_embedding.weight")
    m, r = ln_stats(x, s.ln_eps)
    x = (x - m) * r * T("vision_model.pre_layrnorm.weight") + T("vision_model.pre_layrnorm.bias")
    d, H = s.v_hidden, s.v_heads
    x = x.reshape(-1, d)
    if mode != "fp32":
        x = bf16(x)
    site = [0]

    def proj(xin, g, b_ln, w, bias):
        """LayerNorm(xin) @ w^T + bias in the tower's arithmetic"""
        m, r = ln_stats(xin, s.ln_eps)
        y = (xin - m) * r * g + b_ln
        if mode == "fp32":
            return y @ w.T + bias
        if mode == "fp8":
            return mx_quant(y) @ w_quant(w).T + bias
        if mode == "collect":
            y64 = y.double()
            table.append((y64.mean(dim=0), y64.var(dim=0, unbiased=False)))
            return bf16(y) @ bf16(w).T + bias
        mu = table[site[0]]
        site[0] += 1
        return mx_quant((xin - m) * r * g + (b_ln - mu)) @ w_quant(w).T + (bias + bf16(w) @ mu)

    def plain(xin, w, bias):
        if mode == "fp32":
            return xin @ w.T + bias
        if mode == "collect":
            return bf16(xin) @ bf16(w).T + bias
        return mx_quant(xin) @ w_quant(w).T + bias

    for i in range(s.v_layers):
        p = f"vision_model.encoder.layers.{i}."
        wqkv = torch.cat([T(p + f"self_attn.{n}.weight") for n in ("q_proj", "k_proj", "v_proj")])
        bqkv = torch.cat([T(p + f"self_attn.{n}.bias") for n in ("q_proj", "k_proj", "v_proj")])
        qkv = proj(x, T(p + "layer_norm1.weight"), T(p + "layer_norm1.bias"), wqkv, bqkv)
        if mode != "fp32":
            qkv = bf16(qkv)
        q, k, v = [t.reshape(B, -1, H, 64).transpose(1, 2) for t in qkv.reshape(B, -1, 3 * d).split(d, dim=-1)]
        pr = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, dim=-1)
        ctx = (pr @ v).transpose(1, 2).reshape(-1, d)
        x = x + plain(ctx, T(p + "self_attn.out_proj.weight"), T(p + "self_attn.out_proj.bias"))
        if mode != "fp32":
            x = bf16(x)
        h = proj(x, T(p + "layer_norm2.weight"), T(p + "layer_norm2.bias"), T(p + "mlp.fc1.weight"), T(p + "mlp.fc1.bias"))
        h = h * torch.sigmoid(1.702 * h)
        x = x + plain(h, T(p + "mlp.fc2.weight"), T(p + "mlp.fc2.bias"))
        if mode != "fp32":
            x = bf16(x)
    x0 = x.reshape(B, -1, d)[:, 0]
    m, r = ln_stats(x0, s.ln_eps)
    pooled = (x0 - m) * r * T("vision_model.post_layernorm.weight") + T("vision_model.post_layernorm.bias")
    y = pooled @ T("visual_projection.weight").T
    return torch.nn.functional.normalize(y, dim=-1)


def outlier_weights(W0, how):
    """The seeded weights with the residual outlier channels planted through the position table (None: as they are)."""
    W = dict(W0)
    pos = W["vision_model.embeddings.position_embedding.weight"].copy()
    if how == "all":
        pos[:, 31] += 300.0
        pos[:, 500] -= 180.0
    elif how == "cls":
        pos[0, 31] += 300.0
        pos[0, 500] -= 180.0
    W["vision_model.embeddings.position_embedding.weight"] = pos
    return W


def mu_tables(stats):
    """(mean, variance) per site -> the two tables: every channel centred, and centred by the rule mean^2 >= variance"""
    every = [m.float() for m, _ in stats]
    rule = [torch.where(m * m >= v, m, torch.zeros_like(m)).float() for m, v in stats]
    return every, rule


def run_table(n_images=16, n_cal=16, shape=None, seed=0):
    """{case name: {"today", "every", "rule": 1 - cos vs the fp32 tower, "centred": channels the rule centres over all sites}}"""
    s = shape or co.VIT_B32
    W0 = co.init_weights(s, seed=seed)
    px = np.random.Generator(np.random.Philox(4321)).standard_normal((n_images, 3, s.v_image, s.v_image), dtype=np.float32)
    cpx = np.random.Generator(np.random.Philox(99)).standard_normal((n_cal, 3, s.v_image, s.v_image), dtype=np.float32) * 0.7 + 0.3
    cpx = cpx.astype(np.float32)
    res = {}
    for name, how in CASES:
        W = outlier_weights(W0, how)
        with torch.no_grad():
            ref = tower(px, W, s, "fp32")
            stats = []
            tower(cpx, W, s, "collect", stats)
            every, rule = mu_tables(stats)
            f = lambda t: (1 - (t * ref).sum(-1)).max().item()
            res[name] = {"today": f(tower(px, W, s, "fp8")), "every": f(tower(px, W, s, "centred", every)),
                         "rule": f(tower(px, W, s, "centred", rule)), "centred": int(sum((t != 0).sum() for t in rule))}
    return res


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    print(f"ViT-B/32, {n} images (Philox 4321), calibrated on {n} other images (Philox 99, * 0.7 + 0.3): 1 - cos vs the fp32 tower")
    print(f"{'weights':<34} {'fp8 today':>10} {'every ch.':>10} {'by rule':>10}   channels centred by the rule")
    for name, r in run_table(n, n).items():
        print(f"{name:<34} {r['today']:>10.2e} {r['every']:>10.2e} {r['rule']:>10.2e}   {r['centred']}", flush=True)


if __name__ == "__main__":
    main()
