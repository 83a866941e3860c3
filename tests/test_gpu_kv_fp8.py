"""FP8 (e4m3) K / V cache: the append kernels against the fp32 RoPE and the plain quantisation rule, the decode kernel (one stream and the table form) against
fp64 softmax attention over the SAME dequantised cache, the expansion against bf16(code * scale), and the model switch against the oracle with a fake-quantised
KVCache."""
import ctypes as C
import dataclasses

import pytest
import torch

from oracle import streammind_oracle as O
from oracle.make_golden import TINY_V as TV, TINY_C as TC, TINY_G as TG, TINY_L as TL
from tests.util_models import LOGIT_TOL, conn_gate_weights, path_config

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
H_A, KV_A, SMAX_A = 4, 2, 256            # the append tests' shape
PHASES = (("prefill", 40), ("decode", 24), ("prefill", 300), ("decode", 8))
ORACLE_GAP = 3.7e-2     # see test_model_logits_against_the_oracle
WIDE = (O.ConnCfg(mm_hidden=128, d_model=1024), O.LmCfg.gate(hidden=1024, heads=8, kv_heads=2, mlp=512), dataclasses.replace(TL, hidden=1024, heads=8, kv_heads=2))


@pytest.fixture(scope="module")
def nat():
    from streammind_amd import native, _lib
    _lib.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return native


def rnd(shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def quant_rows(x):
    """the plain rule on rows of 128: scale = amax / 448 (1 for a zero row), codes = (x / s).clamp(+-448) cast to e4m3 (RNE, no NaN after the clamp)"""
    am = x.abs().amax(-1, keepdim=True)
    s = torch.where(am > 0, am / 448.0, torch.ones_like(am))
    return (x / s).clamp(-448, 448).to(F8), s.squeeze(-1)


def pack_cache(k, v, S_max):
    """k, v fp32 [n][KV][128] -> the two buffers of the format (uint8, rest of the capacity zero) + the dequantised k, v (fp64)"""
    n, KV, _ = k.shape
    kq, ks = quant_rows(k)
    vq, vs = quant_rows(v)
    kb = torch.zeros(S_max * KV * 132, dtype=torch.uint8)
    vb = torch.zeros(S_max * KV * 132, dtype=torch.uint8)
    kb[:n * KV * 128] = kq.view(torch.uint8).reshape(-1)
    kb[S_max * KV * 128:].view(torch.float32).view(S_max, KV)[:n] = ks
    vb[:S_max * KV * 128].view(KV, 128, S_max)[:, :, :n] = vq.view(torch.uint8).permute(1, 2, 0)
    vb[S_max * KV * 128:].view(torch.float32).view(KV, S_max)[:, :n] = vs.t()
    return kb, vb, kq.double() * ks.double()[..., None], vq.double() * vs.double()[..., None]


def ref_attention(q, kd, vd, lo=0, got=None):
    """fp64 softmax attention of q [H][128] over keys lo.. of the dequantised cache [n][KV][128]; got given: its error relative to the reference's max"""
    rep = q.shape[0] // kd.shape[1]
    kk, vv = kd[lo:].repeat_interleave(rep, 1), vd[lo:].repeat_interleave(rep, 1)
    p = torch.softmax(torch.einsum("hd,khd->hk", q.double(), kk) * 128 ** -0.5, -1)
    ref = torch.einsum("hk,khd->hd", p, vv)
    return ref if got is None else ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _append(nat, n, pos0, fp8, qkv, cos, sin, kb=None, vb=None):
    q = torch.empty(n, H_A * 128, dtype=torch.bfloat16, device="cuda")
    if kb is None:
        kb, vb = (torch.full((SMAX_A * KV_A * (132 if fp8 else 256),), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2))
    fn = nat._lib.load().sm_rope_kv_append_fp8 if fp8 else nat._lib.load().sm_rope_kv_append
    assert fn(qkv.data_ptr(), n, pos0, H_A, KV_A, 128, cos.data_ptr(), sin.data_ptr(), q.data_ptr(), kb.data_ptr(), vb.data_ptr(), SMAX_A, _st()) == 0
    torch.cuda.synchronize()
    return q, kb, vb


@pytest.mark.parametrize("n,pos0", [(1, 0), (1, 37), (33, 5), (130, 62)])
def test_append(nat, n, pos0):
    cfg = dataclasses.replace(TL, hidden=H_A * 128, heads=H_A, kv_heads=KV_A)
    cos, sin = (t[:, :64].contiguous().cuda() for t in O.rope_cos_sin(torch.arange(SMAX_A), cfg))
    qkv = rnd((n, (H_A + 2 * KV_A) * 128), 100 + n).cuda()
    qkv[0, H_A * 128:(H_A + 1) * 128] = 0                                   # an all-zero K row: scale 1, codes 0
    q8, kb, vb = _append(nat, n, pos0, True, qkv, cos, sin)
    assert torch.equal(q8, _append(nat, n, pos0, False, qkv, cos, sin)[0])
    x = qkv.view(n, H_A + 2 * KV_A, 128)
    c, s = cos[pos0:pos0 + n, None, :], sin[pos0:pos0 + n, None, :]
    a, b = x[:, H_A:H_A + KV_A, :64], x[:, H_A:H_A + KV_A, 64:]
    xk, xv = torch.cat([a * c - b * s, b * c + a * s], -1), x[:, H_A + KV_A:]          # fp32 RoPE
    nc, rows = SMAX_A * KV_A * 128, slice(pos0, pos0 + n)
    kcode, kscale = kb[:nc].view(SMAX_A, KV_A, 128), kb[nc:].view(torch.float32).view(SMAX_A, KV_A)
    vcode, vscale = vb[:nc].view(KV_A, 128, SMAX_A).permute(2, 0, 1), vb[nc:].view(torch.float32).view(KV_A, SMAX_A).t()
    for name, xx, code, scale in (("k", xk, kcode, kscale), ("v", xv, vcode, vscale)):
        am = xx.abs().amax(-1)
        want, sc, cd = torch.where(am > 0, am / 448.0, torch.ones_like(am)), scale[rows], code[rows].contiguous()
        assert ((sc - want).abs() <= torch.nextafter(want, want * 2) - want).all(), name                  # 1 fp32 ulp
        assert not ((cd & 0x7F) == 0x7F).any(), name                       # no NaN code
        deq = cd.view(F8).float() * sc[..., None]
        bound = torch.maximum(xx.abs() * 2.0 ** -4, sc[..., None] * 2.0 ** -10) * (1 + 1e-6)
        assert ((deq - xx).abs() <= bound).all(), (name, ((deq - xx).abs() - bound).max().item())
        keep = torch.ones(SMAX_A, dtype=torch.bool)
        keep[rows] = False
        assert (code[keep] == 0x5A).all() and (scale[keep].contiguous().view(torch.uint8) == 0x5A).all(), name
    if n == 33:                                                              # the tile form against 33 calls of the row form, byte for byte
        kb1, vb1 = torch.full_like(kb, 0x5A), torch.full_like(vb, 0x5A)
        for t in range(n):
            _append(nat, 1, pos0 + t, True, qkv[t:t + 1].contiguous(), cos, sin, kb1, vb1)
        assert torch.equal(kb, kb1) and torch.equal(vb, vb1)


@pytest.fixture(scope="module")
def cache6k():
    out = {}
    for H, KV, n in ((32, 8, 6144), (2, 1, 256)):
        out[(H, KV)] = (rnd((H, 128), 9).bfloat16(), rnd((n, KV, 128), 7), rnd((n, KV, 128), 8))
        out[(H, KV)][1][:, :, :4] *= 6                                      # a few dominant dims, as rotated keys have
    return out


def _decode(nat, q, kb, vb, pos, H, KV, S_max, window=0):
    ws, ctx = torch.empty(32 * H * 130, device="cuda"), torch.empty(H, 128, dtype=torch.bfloat16, device="cuda")
    assert nat._lib.load().sm_llm_decode_attention_fp8(q.data_ptr(), kb.data_ptr(), vb.data_ptr(), pos, H, KV, 128, S_max, window, ws.data_ptr(), 32, ctx.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    return ctx.cpu()


@pytest.mark.parametrize("pos,H,KV,W", [(p, 32, 8, 0) for p in (0, 31, 32, 37, 383, 384, 511, 513, 2047, 2048, 4095)] + [(200, 2, 1, 0), (63, 32, 8, 64), (700, 32, 8, 33), (5000, 32, 8, 4096)])
def test_decode_attention(nat, cache6k, pos, H, KV, W):
    q, k, v = cache6k[(H, KV)]
    S_max = 6144 if W else 4096
    kb, vb, kd, vd = pack_cache(k[:pos + 1], v[:pos + 1], S_max)
    got = _decode(nat, q.cuda(), kb.cuda(), vb.cuda(), pos, H, KV, S_max, W)
    assert ref_attention(q, kd, vd, max(0, pos + 1 - W) if W else 0, got) < 8e-3
    if W > pos:
        assert torch.equal(got, _decode(nat, q.cuda(), kb.cuda(), vb.cuda(), pos, H, KV, S_max))
    nc, dead = S_max * KV * 128, torch.arange(S_max) > (pos if pos < 384 else S_max)             # NaN codes and NaN scales behind pos (pos < 384) ...
    dead |= torch.arange(S_max) < (pos + 1 - W if W else 0)                                      # ... and in front of the window must not reach the output
    if dead.any():
        kb[:nc].view(S_max, KV * 128)[dead] = 0x7F
        kb[nc:].view(torch.float32).view(S_max, KV)[dead] = float("nan")
        vb[:nc].view(KV * 128, S_max)[:, dead] = 0x7F
        vb[nc:].view(torch.float32).view(KV, S_max)[:, dead] = float("nan")
        assert torch.equal(got, _decode(nat, q.cuda(), kb.cuda(), vb.cuda(), pos, H, KV, S_max, W))


@pytest.mark.parametrize("S", [3, 40, 130])
def test_decode_attention_many_streams(nat, cache6k, S):
    H, KV, S_max = 32, 8, 2048
    _, k, v = cache6k[(H, KV)]
    pos = [2047] + [[0, 31, 32, 200, 511, 2047][int(i)] for i in torch.randint(0, 6, (S - 1,), generator=torch.Generator().manual_seed(S))]
    packs = {p: pack_cache(k[:p + 1], v[:p + 1], S_max) for p in set(pos)}                  # streams at one position share one cache
    dev = {p: (packs[p][0].cuda(), packs[p][1].cuda()) for p in packs}
    q = rnd((S, H, 128), 50 + S).bfloat16()
    kt, vt = (torch.tensor([dev[p][j].data_ptr() for p in pos], dtype=torch.int64).cuda() for j in (0, 1))
    pd, qd = torch.tensor(pos, dtype=torch.int32).cuda(), q.cuda()
    ws, ctx = torch.empty(64 * H * 130, device="cuda"), torch.empty(S, H, 128, dtype=torch.bfloat16, device="cuda")
    assert nat._lib.load().sm_llm_decode_attention_fp8_tab(qd.data_ptr(), kt.data_ptr(), vt.data_ptr(), pd.data_ptr(), S, 2048, H, KV, 128, S_max, 0, ws.data_ptr(), 64,
                                                          ctx.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    for t, p in enumerate(pos):
        assert ref_attention(q[t], packs[p][2], packs[p][3], 0, ctx[t].cpu()) < 8e-3, (t, p)


@pytest.mark.parametrize("k_lo,k_hi", [(0, 1), (5, 70), (64, 256)])
def test_expand(nat, k_lo, k_hi):
    KV, S_max = 2, 256
    kb, vb, _, _ = pack_cache(rnd((S_max, KV, 128), 3), rnd((S_max, KV, 128), 4), S_max)
    ko, vo = (torch.full(sh, 7.0, dtype=torch.bfloat16, device="cuda") for sh in ((S_max, KV * 128), (KV * 128, S_max)))
    kd, vd = kb.cuda(), vb.cuda()
    assert nat._lib.load().sm_kv_fp8_expand(kd.data_ptr(), vd.data_ptr(), k_lo, k_hi, KV, 128, S_max, ko.data_ptr(), vo.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    nc = S_max * KV * 128
    kw = (kb[:nc].view(F8).float().view(S_max, KV, 128) * kb[nc:].view(torch.float32).view(S_max, KV, 1)).bfloat16().view(S_max, KV * 128)
    vw = (vb[:nc].view(F8).float().view(KV, 128, S_max) * vb[nc:].view(torch.float32).view(KV, 1, S_max)).bfloat16().view(KV * 128, S_max)
    kw[:k_lo] = 7.0; kw[k_hi:] = 7.0; vw[:, :k_lo] = 7.0; vw[:, k_hi:] = 7.0
    assert torch.equal(ko.cpu(), kw) and torch.equal(vo.cpu(), vw)


def _tiny_model(nat, Wl, cfgs=(TC, TG, TL), **kw):
    m = nat.NativeModel(dataclasses.replace(path_config(TV, *cfgs), **kw))
    named = [("model.vision_tower.vision_tower.vision_model." + k, v) for k, v in O.make_vit_weights(TV, 41).items()]
    named += [("model.mm_projector." + k, v) for k, v in conn_gate_weights(*cfgs[:2], 86).items()] + list(Wl.items())
    for k, v in named:
        m.load_tensor(k, v.to(torch.bfloat16) if v.dim() >= 2 and "conv1d" not in k and "A_log" not in k else v.float())
    assert m.missing() == []
    m.finalize()
    return m


def oracle_logits(Wl, ids, fake_quant):
    """the pending logits after each phase from oracle.lm_forward (mixed precision) driven over `ids`; fake_quant: the rows a call appended to its KVCache are
    replaced by their fp8 dequantisation (the plain rule) after that call"""
    table = Wl["model.embed_tokens.weight"].bfloat16().float()
    cache, out, done = O.KVCache(), [], 0
    for kind, n in PHASES:
        for rows in ([n] if kind == "prefill" else [1] * n):
            lg = O.lm_forward(table[ids[done:done + rows].long()], Wl, TL, cache, prec=O.MIXED)
            for lst in (cache.k, cache.v) if fake_quant else ():
                for l in range(len(lst)):
                    c, s = quant_rows(lst[l][done:])
                    lst[l] = torch.cat([lst[l][:done], c.float() * s[..., None]])
            done += rows
        out.append(lg)
    return out


def test_model_logits_against_the_oracle(nat):
    """kv_fp8 on the tiny Mistral (head_dim 128): a 40-token prefill, 24 decode steps, a 300-token prefill that reads the existing cache through the expansion,
    8 more steps, every token teacher-forced; the pending logits after each phase against the oracle whose KVCache rows are fake-quantised after the call that
    appended them.  That reference sees a call's own rows unquantised (the GPU path does not), so the bound is LOGIT_TOL (3e-2) + ORACLE_GAP: the largest
    distance between that oracle run and the plain one over the four phases, computed on the CPU with oracle_logits for this seed (per phase 0 / 3.61e-2 /
    1.66e-2 / 2.34e-2 on logits of magnitude 2.6 .. 4.0) -- 3.61e-2, rounded up to 3.7e-2.  And what kv_bytes() reports in both modes."""
    Wl = O.make_lm_weights(TL, 44)
    ids = torch.randint(3, TL.vocab, (sum(n for _, n in PHASES),), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    ref = oracle_logits(Wl, ids, True)
    s, s16 = (_tiny_model(nat, Wl, kv_fp8=on).open_stream(max_frames=8, max_seq=1024) for on in (True, False))
    L, KV, dh = TL.layers, TL.kv_heads, TL.head_dim
    assert s.kv_bytes() == L * s.kv_capacity * (2 * KV * dh + 8 * KV) and s16.kv_bytes() == L * s16.kv_capacity * 4 * KV * dh
    done = 0
    for ph, (kind, n) in enumerate(PHASES):
        if kind == "prefill":
            s.prefill(ids[done:done + n].cuda())
        else:
            for t in range(n):
                s.set_next_token(ids[done + t:done + t + 1].cuda())
                s.decode(1)
        done += n
        d = (s.logits()[0].float().cpu() - ref[ph]).abs().max().item()
        assert d < LOGIT_TOL + ORACLE_GAP, (ph, d)
    assert s.kv_len == done and s.kv_bytes() == L * s.kv_capacity * (2 * KV * dh + 8 * KV)


@pytest.mark.parametrize("S,cfgs", [(3, (TC, TG, TL)), (70, WIDE)])
def test_model_group_decode_equals_solo(nat, S, cfgs):
    """sm_group_llm_decode on the fp8 cache (table forms of append and attention) emits, for 8 steps, exactly the ids sm_llm_decode emits for each stream alone, on
    the planted-margin weights of test_gpu_parity_full (every solo step's top-2 margin is asserted above 4 x the logit tolerance: no near-tie allowance).  3 streams
    with one context; 70 streams with contexts of 5..59 tokens at hidden 1024, where a step's q|k|v product leaves split-K slabs that the append kernel sums."""
    from tests.test_gpu_parity_full import _planted_llm
    m = _tiny_model(nat, _planted_llm(cfgs[2], 808, peak=16.0)[0], cfgs, kv_fp8=True)
    g = torch.Generator().manual_seed(12)
    ctxs = [torch.randint(3, cfgs[2].vocab, (int(torch.randint(5, 60, (1,), generator=g)),), generator=g, dtype=torch.int32).cuda() for _ in range(S)]
    ctxs = [ctxs[0]] * 3 if S == 3 else ctxs
    want, streams = [], []
    for solo in (True, False):
        for c in ctxs:
            s = m.open_stream(max_frames=8, max_seq=128)
            s.prefill(c)
            if solo:
                want.append([])
                for _ in range(8):
                    assert float(torch.topk(s.logits()[0], 2).values.diff().abs()) > 4 * LOGIT_TOL
                    want[-1].append(int(s.decode(1)[0]))
            else:
                streams.append(s)
    assert m.open_group(streams).decode(8).cpu().tolist() == want


def test_model_cache_growth_keeps_codes_and_scales(nat):
    """a 500-token prefill, then 30 more tokens: the second call grows the cache 512 -> 1024 (codes and scales move separately, the scale offset depends on the
    capacity).  Against one 530-token prefill, whose cache grew while empty: the same logits within the logit tolerance (the chunking differs, the cache must not)."""
    m = _tiny_model(nat, O.make_lm_weights(TL, 44), kv_fp8=True)
    ids = torch.randint(3, TL.vocab, (530,), generator=torch.Generator().manual_seed(6), dtype=torch.int32).cuda()
    a, b = (m.open_stream(max_frames=8, max_seq=1024) for _ in range(2))
    a.prefill(ids[:500]); a.prefill(ids[500:]); b.prefill(ids)
    assert a.kv_capacity == b.kv_capacity == 1024 and a.kv_bytes() == b.kv_bytes()
    assert (a.logits()[0] - b.logits()[0]).abs().max().item() < LOGIT_TOL


def test_refusals(nat):
    lib = nat._lib.load()
    f16 = nat.NativeModel(dataclasses.replace(path_config(TV, TC, TG, TL), llm_fp16=True))
    assert lib.sm_model_set_kv_fp8(f16.h, 1) == -1 and b"llm_fp16" in lib.sm_last_error()
    m = _tiny_model(nat, O.make_lm_weights(TL, 44))
    assert lib.sm_model_set_kv_fp8(m.h, 2) == -1 and b"on = 2" in lib.sm_last_error()
    assert lib.sm_model_set_kv_fp8(m.h, 1) == 0 and lib.sm_model_set_kv_fp8(m.h, 0) == 0
    s = m.open_stream(max_frames=8, max_seq=64)
    assert s.kv_len == 0 and lib.sm_model_set_kv_fp8(m.h, 1) == -1 and b"sm_stream_open" in lib.sm_last_error()
