"""MXFP4 weights above 128 rows (SM_W_FP4_GEMM, `w_fp4=3` / `weights_fp4=2, fp4_gemm=True`): the activation prepass + tiled fp4 GEMM against fp64 on the
exact dequantised weights, its boundaries against SM_W_FP4_MFMA / SM_W_FP4, and the model switch (a 160-token prefill chunk, then decode steps)."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import streammind_oracle as O
from oracle.make_golden import TINY_V as TV, TINY_C as TC, TINY_G as TG, TINY_L as TL
from tests.util_models import conn_gate_weights, path_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from streammind_amd import native, _lib
    _lib.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return native


def rnd(shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _products(x64, wd, wd2, bias, res):
    y = x64 @ wd.T
    if wd2 is not None:
        return O.silu(torch.from_numpy(y)).numpy() * (x64 @ wd2.T)
    if bias is not None:
        y = O.silu(torch.from_numpy(y + bias)).numpy() + res
    return y


# 129: three 64-row tiles, the last with one row; 192: whole 64-row tiles; 257: three 128-row tiles, the last with one row (128-row tiles start above 256 rows)
CASES = [(M, N, K, form, xdt) for M in (129, 192, 257) for N, K in ((17, 160), (272, 1024), (256, 4096)) for form in ("plain", "epilogue", "dual")
         for xdt in (torch.float32, torch.bfloat16)]
CASES += [(129, 32, 14336, "dual", torch.bfloat16)]         # Mistral's down-projection depth: the steady state of the LDS ring, seven K slabs


@pytest.mark.parametrize("M,N,K,form,xdt", CASES)
def test_linear_fp4_above_128_rows(nat, M, N, K, form, xdt):
    """The rule of test_linear_fp4_17_to_128_rows: fp64 of the fp32 master x on the exact dequantised weights; the max-abs error is at most 4 x e16, e16 = the
    error of the same fp64 product with x rounded to bf16.  fp32 rows additionally stay under 0.75 x e16 (hi + lo carries 2^-9 of the binade, bf16 2^-8):
    the expansion path, which rounds x to bf16, sits at 1.0 -- and refuses fp32 rows above 128 in the first place."""
    x = rnd((M, K), 2 + M)
    x[0, 5] *= 40.0; x[M - 1, K - 32:] *= 1e-3                                  # blocks of very different magnitude: the x scales are per 32-block
    w, w2 = rnd((N, K), 1, K ** -0.5).bfloat16(), rnd((N, K), 5, K ** -0.5).bfloat16()
    wp, w2p = nat.pack_weight_fp4(w.cuda()), nat.pack_weight_fp4(w2.cuda())
    wd = nat.unpack_weight_fp4(wp, N, K).double().cpu().numpy()
    wd2 = nat.unpack_weight_fp4(w2p, N, K).double().cpu().numpy() if form == "dual" else None
    bias, res = (rnd((N,), 3, 0.1), rnd((M, N), 4)) if form == "epilogue" else (None, None)
    b64, r64 = (bias.double().numpy(), res.double().numpy()) if bias is not None else (None, None)
    ref = _products(x.double().numpy(), wd, wd2, b64, r64)
    e16 = np.abs(_products(x.bfloat16().double().numpy(), wd, wd2, b64, r64) - ref).max()
    xg = x.cuda().to(xdt)
    out16 = None
    if form == "plain":
        y = nat.linear(xg, wp, N, K, w_fp4=3)
    elif form == "epilogue":
        out16 = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        rg = res.cuda()
        y = nat.linear(xg, wp, N, K, w_fp4=3, bias=bias.cuda(), act=4, residual=rg, out=rg, out16=out16)      # the residual aliases the fp32 output
    else:
        y = nat.linear(xg, wp, N, K, w2p=w2p, w_fp4=3)
    err = np.abs(y.double().cpu().numpy() - ref).max()
    print(f"fp4 gemm M={M} N={N} K={K} {form} {xdt}: err {err:.3e} e16 {e16:.3e} ratio {err / e16:.3f}")
    assert err <= 4 * e16, (err, e16)
    if xdt == torch.float32:
        assert err <= 0.75 * e16, (err, e16)
    if out16 is not None:
        assert torch.equal(out16, y.bfloat16())


@pytest.mark.parametrize("M,kw,other", [(128, {}, 2), (200, dict(precise=True), True), (200, {}, 3)])
def test_fp4_gemm_boundaries(nat, M, kw, other):
    """128 rows: SM_W_FP4_MFMA's kernel; a field the tiled kernel does not carry: the expansion; the tiled kernel twice: the same bits (fixed slab order)"""
    N, K = 48, 1024
    x = rnd((M, K), 2).bfloat16().cuda()                                        # (the tiled kernels of the expansion take 16-bit rows)
    wp = nat.pack_weight_fp4(rnd((N, K), 1, K ** -0.5).bfloat16().cuda())
    assert torch.equal(nat.linear(x, wp, N, K, w_fp4=3, **kw), nat.linear(x, wp, N, K, w_fp4=other, **kw))


def _tiny_model(nat, Wl, fp4, gemm=False):
    m = nat.NativeModel(dataclasses.replace(path_config(TV, TC, TG, TL), weights_fp4=fp4, fp4_gemm=gemm))
    for k, v in O.make_vit_weights(TV, 41).items():
        m.load_tensor("model.vision_tower.vision_tower.vision_model." + k, v.to(torch.bfloat16) if v.dim() >= 2 else v)
    for k, v in conn_gate_weights(TC, TG, 86).items():
        m.load_tensor("model.mm_projector." + k, v.to(torch.bfloat16) if v.dim() >= 2 and "conv1d" not in k and "A_log" not in k else v)
    for k, v in Wl.items():
        m.load_tensor(k, v.to(torch.bfloat16) if v.dim() >= 2 else v)
    assert m.missing() == []
    m.finalize()
    return m


def test_model_fp4_gemm_prefill(nat):
    """sm_model_set_fp4_gemm needs mode 2 and takes 0 / 1 only; with it on, a 160-token prefill (every fp4 product above 128 rows; the tiny widths make K one
    ragged k-step) + 2 decode steps stay within 3e-2 of the bf16 model on the dequantised weights, ids equal."""
    Wl = O.make_lm_weights(TL, 44)
    fresh = nat.NativeModel(path_config(TV, TC, TG, TL))                        # before the first tensor: only the switches decide
    assert fresh.lib.sm_model_set_fp4_gemm(fresh.h, 1) == -1
    assert fresh.lib.sm_model_set_weights_fp4(fresh.h, 2) == 0
    assert [fresh.lib.sm_model_set_fp4_gemm(fresh.h, on) for on in (2, 1, 0)] == [-1, 0, 0]
    m4 = _tiny_model(nat, Wl, 2, True)
    Wd = {k: (nat.unpack_weight_fp4(nat.pack_weight_fp4(v.bfloat16().cuda()), *v.shape).float().cpu() if ".layers." in k and v.dim() == 2 else v) for k, v in Wl.items()}
    ids = (torch.arange(160, dtype=torch.int32) * 7 + 3) % TL.vocab
    s4, sd = m4.open_stream(max_frames=8, max_seq=256), _tiny_model(nat, Wd, 0).open_stream(max_frames=8, max_seq=256)
    for step in range(3):                                       # the prefill, then two decode steps teacher-forced with the bf16 model's tokens
        if step == 0:
            s4.prefill(ids.cuda()); sd.prefill(ids.cuda())
        else:
            s4.set_next_token(sd.logits()[1])
            assert s4.decode(1).cpu().tolist() == sd.decode(1).cpu().tolist()
        assert (s4.logits()[0].float() - sd.logits()[0].float()).abs().max() < 3e-2, step
