"""The twin rule of the `*_bf16` HBM-bound kernels, shared by the GPU test modules: each twin runs the SAME fp32
arithmetic as its `*_f32` original on widened inputs and rounds once on store.  On bf16-representable inputs therefore a
stored result == round_to_bf16(float result), bit for bit."""
import torch

BF = torch.bfloat16


def _pair(shape, seed, scale=1.0):
    """the same random bf16-representable tensor on the device, stored as bfloat16 and as float32"""
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(*shape, generator=g) * scale).to(BF).cuda()
    return h, h.float()


def _same_stored(h_out, f_out, what):
    assert h_out.dtype == BF and f_out.dtype == torch.float32
    assert torch.equal(h_out, f_out.to(BF)), f"{what}: bf16 kernel != round(float kernel), max diff {float((h_out.float() - f_out).abs().max()):.3e}"
