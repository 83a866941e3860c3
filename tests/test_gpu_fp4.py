"""MXFP4 LLM weights (SM_W_FP4): the quantiser against a numpy restatement of its rule, the <= 16-row block-scaled MFMA kernel and the
expanded > 16-row path against fp64 on the exact dequantised weights, the model switch against a bf16 model holding those weights."""
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


def mxfp4_ref(w):
    """OCP MX v1.0 MXFP4 of fp32 [N, K] (K padded with zeros to whole 32-blocks): X = 2^(floor(log2 max|w|) - 2) per block of 32 along k as an e8m0
    byte (all-zero block: 127), elements RNE(w / X) onto {0, .5, 1, 1.5, 2, 3, 4, 6} saturating at 6 -> the dequantised values, float64 [N, K]."""
    N, K = w.shape
    b = np.zeros((N, -(-K // 32) * 32)); b[:, :K] = w
    b = b.reshape(N, -1, 32)
    am = np.abs(b).max(-1, keepdims=True)
    e = np.where(am > 0, np.floor(np.log2(np.where(am > 0, am, 1.0))) - 2 + 127, 127).clip(0, 254)
    t = np.abs(b) / 2.0 ** (e - 127)
    q = np.where(t < 2, np.rint(t * 2) / 2, np.where(t < 4, np.rint(t), np.rint(t / 2) * 2)).clip(max=6.0)     # np.rint: ties to even = the even code
    return (np.sign(b) * q * 2.0 ** (e - 127)).reshape(N, -1)[:, :K]


@pytest.mark.parametrize("N,K", [(16, 128), (17, 160), (40, 1024)])
def test_quantiser_is_the_mx_rule(nat, N, K):
    w = rnd((N, K), 7 + N, K ** -0.5).bfloat16()
    w[3, 32:64] = 0                                                            # an all-zero block
    w[5, 64] = 7.5 * 2.0 ** -3; w[5, 65:96] *= 0.1                             # a maximum that saturates to 6 (X = 2^-3)
    w[9, 0:32] = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -2.5, -5.0] + [0.0] * 21).bfloat16() * 2.0 ** -5   # ties, X = 2^-5
    wp = nat.pack_weight_fp4(w.cuda())
    assert wp.numel() == nat._lib.load().sm_packed_fp4_bytes(N, K) == -(-N // 16) * (-(-K // 128) * 1024 + -(-K // 512) * 256)
    got = nat.unpack_weight_fp4(wp, N, K).float().cpu().numpy().astype(np.float64)
    ref = mxfp4_ref(w.float().numpy())
    assert ref[3, 32:64].max() == 0 and abs(ref[5, 64]) == 6 * 2.0 ** -3 and ref[9, 1] == 0 and ref[9, 5] == 2 * 2.0 ** -5 and ref[9, 7] == 4 * 2.0 ** -5
    assert np.array_equal(got, ref)


def _products(x64, wd, wd2, bias, res):
    y = x64 @ wd.T
    if wd2 is not None:
        return O.silu(torch.from_numpy(y)).numpy() * (x64 @ wd2.T)
    if bias is not None:
        y = O.silu(torch.from_numpy(y + bias)).numpy() + res
    return y


# every (M, shape, form, x type); the fused RMSNorm exists for fp32 rows within its M*K <= 16384 limit
CASES = [(M, N, K, form, xdt) for M in (1, 7, 16) for N, K in ((17, 160), (48, 1024), (256, 4096)) for form in ("plain", "epilogue", "dual", "norm")
         for xdt in (torch.float32, torch.bfloat16) if form != "norm" or (xdt == torch.float32 and M * K <= 16384)]
# + Mistral's down-projection depth: enough k-steps per wave for the steady state of the register ring (K = 4096 ends in its short form)
CASES += [(1, 32, 14336, "plain", torch.bfloat16), (2, 32, 14336, "dual", torch.float32)]


@pytest.mark.parametrize("M,N,K,form,xdt", CASES)
def test_linear_fp4_up_to_16_rows(nat, M, N, K, form, xdt):
    """fp64 of the fp32 master x on the exact dequantised weights (the kernel is fed that x, or its bf16 rounding); the kernel's max-abs error is at most 4 x e16, e16 = the error of the same fp64 product with x
    rounded to bf16 (2: truncation instead of rounding in a hi/lo split; 2: the lo term's rounding + fp32 accumulation).  A dropped lo term sits near 16 x e16.
    norm_gamma: x is the residual stream, the operand that is rounded is gamma * x * rstd."""
    x = rnd((M, K), 2 + M)
    x[0, 5] *= 40.0; x[M - 1, K - 32:] *= 1e-3                                  # blocks of very different magnitude: the x scales are per 32-block
    w, w2 = rnd((N, K), 1, K ** -0.5).bfloat16(), rnd((N, K), 5, K ** -0.5).bfloat16()
    wp, w2p = nat.pack_weight_fp4(w.cuda()), nat.pack_weight_fp4(w2.cuda())
    wd = nat.unpack_weight_fp4(wp, N, K).double().cpu().numpy()
    wd2 = nat.unpack_weight_fp4(w2p, N, K).double().cpu().numpy() if form == "dual" else None
    bias, res = (rnd((N,), 3, 0.1), rnd((M, N), 4)) if form == "epilogue" else (None, None)
    gamma = 1.0 + rnd((K,), 6, 0.1)
    xop = x.double()
    if form == "norm":
        xop = gamma.double() * (xop * torch.rsqrt((xop * xop).mean(-1, keepdim=True) + 1e-5))
    b64, r64 = (bias.double().numpy(), res.double().numpy()) if bias is not None else (None, None)
    ref = _products(xop.numpy(), wd, wd2, b64, r64)
    e16 = np.abs(_products(xop.float().bfloat16().double().numpy(), wd, wd2, b64, r64) - ref).max()
    xg = x.cuda().to(xdt)
    out16 = None
    if form == "plain":
        y = nat.linear(xg, wp, N, K, w_fp4=True)
    elif form == "epilogue":
        out16 = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        rg = res.cuda()
        y = nat.linear(xg, wp, N, K, w_fp4=True, bias=bias.cuda(), act=4, residual=rg, out=rg, out16=out16)      # the residual aliases the fp32 output
    elif form == "dual":
        y = nat.linear(xg, wp, N, K, w2p=w2p, w_fp4=True)
    else:
        y = nat.linear(xg, wp, N, K, w_fp4=True, norm_gamma=gamma.cuda(), norm_eps=1e-5)
    err = np.abs(y.double().cpu().numpy() - ref).max()
    print(f"fp4 M={M} N={N} K={K} {form} {xdt}: err {err:.3e} e16 {e16:.3e} ratio {err / e16:.3f}")
    assert err <= 4 * e16, (err, e16)
    if out16 is not None:
        assert torch.equal(out16, y.bfloat16())


@pytest.mark.parametrize("M", [17, 40])
def test_linear_fp4_more_than_16_rows(nat, M):
    """the image expanded to packed bf16 (exact) + the bf16 kernels: their definition to 1e-5 relative, as the expanded branch of the fp8 test"""
    N, K = 48, 1024
    x = rnd((M, K), 2).bfloat16()
    wp = nat.pack_weight_fp4(rnd((N, K), 1, K ** -0.5).bfloat16().cuda())
    bias = rnd((N,), 3, 0.1)
    ref = x.double() @ nat.unpack_weight_fp4(wp, N, K).double().cpu().t() + bias.double()
    y = nat.linear(x.cuda(), wp, N, K, w_fp4=True, bias=bias.cuda())
    assert ((y.double().cpu() - ref).abs().max() / ref.abs().max()).item() < 1e-5


def _tiny_model(nat, Wl, fp4):
    m = nat.NativeModel(dataclasses.replace(path_config(TV, TC, TG, TL), weights_fp4=fp4))
    for k, v in O.make_vit_weights(TV, 41).items():
        m.load_tensor("model.vision_tower.vision_tower.vision_model." + k, v.to(torch.bfloat16) if v.dim() >= 2 else v)
    for k, v in conn_gate_weights(TC, TG, 86).items():
        m.load_tensor("model.mm_projector." + k, v.to(torch.bfloat16) if v.dim() >= 2 and "conv1d" not in k and "A_log" not in k else v)
    for k, v in Wl.items():
        m.load_tensor(k, v.to(torch.bfloat16) if v.dim() >= 2 else v)
    assert m.missing() == []
    m.finalize()
    return m


def test_model_fp4_is_the_bf16_model_on_the_dequantised_weights(nat):
    """the tiny Mistral with weights_fp4 against a plain bf16 model loaded with unpack(pack(W)) for the LLM's q, k, v, o, gate, up, down: a 40-token prefill (chunks
    above 16 rows: the expanded images) + 8 decode steps (the fp4 weight stream: norm_gamma, the gate | up dual image, the RoPE and norm launches of their own), both
    fed the same tokens; the logits after the prefill and after every step within 3e-2, the bound of the weights_fp8 path test."""
    Wl = O.make_lm_weights(TL, 44)
    Wd = {k: (nat.unpack_weight_fp4(nat.pack_weight_fp4(v.bfloat16().cuda()), *v.shape).float().cpu() if ".layers." in k and v.dim() == 2 else v) for k, v in Wl.items()}
    assert sum(not torch.equal(Wd[k], Wl[k]) for k in Wl) == 7 * TL.layers
    ids = (torch.arange(40, dtype=torch.int32) * 7 + 3) % TL.vocab
    s4, sd = [m.open_stream(max_frames=8, max_seq=128) for m in (_tiny_model(nat, Wl, True), _tiny_model(nat, Wd, False))]
    logits = []
    for step in range(9):                                       # the prefill, then eight decode steps teacher-forced with the bf16 model's tokens
        if step == 0:
            s4.prefill(ids.cuda()); sd.prefill(ids.cuda())
        else:
            s4.set_next_token(sd.logits()[1])
            assert s4.decode(1).cpu().tolist() == sd.decode(1).cpu().tolist()
        logits.append((s4.logits()[0].float().cpu(), sd.logits()[0].float().cpu()))
        assert (logits[-1][0] - logits[-1][1]).abs().max() < 3e-2, step
    assert s4.kv_len == sd.kv_len == 48
    assert (logits[0][0] - _prefill_logits(nat, Wl, ids)).abs().max() > 1e-3          # it really is a quantised model


def _prefill_logits(nat, Wl, ids):
    s = _tiny_model(nat, Wl, False).open_stream(max_frames=8, max_seq=128)
    s.prefill(ids.cuda())
    return s.logits()[0].float().cpu()


def test_fp4_refusals(nat):
    """what the fp4 kernel does not do is SM_EINVAL, never a different product; the model switch is fixed before the first tensor"""
    from streammind_amd._lib import StreamMindHipError
    N, K = 32, 256
    wp = nat.pack_weight_fp4(rnd((N, K), 1).bfloat16().cuda())
    x = rnd((4, K), 2).cuda()
    ln_out = torch.empty(4, N, device="cuda")
    for kw, xx in [(dict(precise=True), x), (dict(x_rep=(2, 64)), x[:, :K // 2].contiguous()), (dict(), x.half()),
                   (dict(post_ln=(torch.ones(N, device="cuda"), None, 1e-5, ln_out)), x)]:
        with pytest.raises(StreamMindHipError, match=r"\(-1\)"):
            nat.linear(xx, wp, N, K, w_fp4=True, **kw)
    with pytest.raises(StreamMindHipError, match=r"\(-1\)"):
        nat.NativeModel(dataclasses.replace(path_config(TV, TC, TG, TL, weights_fp8=True), weights_fp4=True))
    m = nat.NativeModel(path_config(TV, TC, TG, TL))
    m.load_tensor("model.norm.weight", torch.ones(TL.hidden))
    assert m.lib.sm_model_set_weights_fp4(m.h, 1) == -1
    m4 = _tiny_model(nat, O.make_lm_weights(TL, 44), True)
    streams = [m4.open_stream(max_frames=8, max_seq=64) for _ in range(17)]
    for s in streams:
        s.prefill(torch.tensor([1, 5, 9], dtype=torch.int32).cuda())
    g = m4.open_group(streams)
    solo = m4.open_stream(max_frames=8, max_seq=64)
    solo.prefill(torch.tensor([1, 5, 9], dtype=torch.int32).cuda())
    tok = solo.decode(1).cpu().tolist()
    out = g.decode(1, active=[True] * 16 + [False]).cpu()                       # 16 active streams: one pass of the fp4 weight stream at 16 rows
    assert out[:16].tolist() == [tok] * 16 and out[16].tolist() == [-1]
    for s in streams[:16]:                                                      # (3e-2: the bound the batched decode tests of the bf16 path use against solo streams)
        assert (s.logits()[0] - solo.logits()[0]).abs().max() < 3e-2
    with pytest.raises(StreamMindHipError, match=r"\(-1\)"):
        g.decode(1)
