"""Fused chunk attention over the FP8 K / V cache (sm_llm_attention_fp8, kv_fp8_chunk): the operator against fp64 causal / windowed softmax attention over the
SAME dequantised cache, with NaN codes and NaN scales planted wherever the call may not look; the model switch against the oracle of test_gpu_kv_fp8."""
import ctypes as C

import pytest
import torch

from oracle import streammind_oracle as O
from oracle.make_golden import TINY_L as TL
from tests.test_gpu_kv_fp8 import ORACLE_GAP, PHASES, _tiny_model, oracle_logits, pack_cache, quant_rows, rnd  # noqa: F401  (quant_rows: the rule pack_cache applies)
from tests.util_models import LOGIT_TOL

pytestmark = pytest.mark.gpu
CASES = [(1, 0, 32, 8, 0), (5, 0, 32, 8, 0), (33, 31, 32, 8, 0), (130, 62, 32, 8, 0), (300, 0, 32, 8, 0), (16, 3000, 32, 8, 0), (70, 200, 2, 1, 0), (40, 20, 2, 2, 0),
         (20, 100, 8, 1, 0), (40, 100, 32, 8, 33), (16, 5000, 32, 8, 4096), (40, 1000, 32, 8, 0)]       # the last: two query tiles AND the key split


@pytest.fixture(scope="module")
def nat():
    from streammind_amd import native, _lib
    _lib.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return native


@pytest.fixture(scope="module")
def qkv():
    """per (H, KV): q [n_max][H][128] bf16, k / v [keys][KV][128] with a few dominant dims in k, as rotated keys have -- made once, shared, never written"""
    out = {}
    for H, KV in {c[2:4] for c in CASES}:
        keys = max(c[0] + c[1] for c in CASES if c[2:4] == (H, KV))
        out[(H, KV)] = (rnd((300, H, 128), 9).bfloat16(), rnd((keys, KV, 128), 7), rnd((keys, KV, 128), 8))
        out[(H, KV)][1][:, :, :4] *= 6
    return out


def ref_chunk(q, kd, vd, pos0, W):
    """fp64 softmax attention of q [n][H][128] at positions pos0.. over the dequantised cache [pos0 + n][KV][128]: key k visible to position p iff p - W < k <= p"""
    rep, qp, kp = q.shape[1] // kd.shape[1], torch.arange(q.shape[0])[:, None] + pos0, torch.arange(kd.shape[0])[None]
    s = torch.einsum("nhd,khd->nhk", q.double(), kd.repeat_interleave(rep, 1)) * 128 ** -0.5
    p = torch.softmax(s.masked_fill(((kp > qp) | ((kp <= qp - W) & (W > 0)))[:, None], float("-inf")), -1)
    return torch.einsum("nhk,khd->nhd", p, vd.repeat_interleave(rep, 1))


def _run(nat, q, kb, vb, n, pos0, H, KV, S_max, W, ws=True):
    w, ctx = torch.empty(16 * 1024 * 130, device="cuda"), torch.empty(n, H, 128, dtype=torch.bfloat16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert nat._lib.load().sm_llm_attention_fp8(q.data_ptr(), kb.data_ptr(), vb.data_ptr(), n, pos0, H, KV, 128, S_max, W, w.data_ptr() if ws else None, w.numel() if ws else 0,
                                                ctx.data_ptr(), st) == 0
    torch.cuda.synchronize()
    return ctx.cpu()


@pytest.mark.parametrize("n,pos0,H,KV,W", CASES)
def test_operator(nat, qkv, n, pos0, H, KV, W):
    q, k, v = qkv[(H, KV)]
    nk, q = pos0 + n, q[:n].contiguous()
    S_max = 6144 if W == 4096 else -(-nk // 64) * 64
    kb, vb, kd, vd = pack_cache(k[:nk], v[:nk], S_max)
    ref = ref_chunk(q, kd, vd, pos0, W)
    err = lambda got: ((got.double() - ref).abs().max() / ref.abs().max()).item()
    got = _run(nat, q.cuda(), kb.cuda(), vb.cuda(), n, pos0, H, KV, S_max, W)
    print(f"chunk_attn_fp8 {(n, pos0, H, KV, W)}: rel err {err(got):.2e}")
    assert err(got) < 8e-3
    if (n, pos0) == (16, 3000):                                   # the same shape without a workspace: one split
        assert err(_run(nat, q.cuda(), kb.cuda(), vb.cuda(), n, pos0, H, KV, S_max, W, ws=False)) < 8e-3
    nc, pos = S_max * KV * 128, torch.arange(S_max)
    dead = (pos >= nk) | ((pos < pos0 - W + 1) & (W > 0))         # NaN codes and NaN scales wherever no query of the call may look: bit-identical output
    if dead.any():
        kb[:nc].view(S_max, KV * 128)[dead] = 0x7F
        kb[nc:].view(torch.float32).view(S_max, KV)[dead] = float("nan")
        vb[:nc].view(KV * 128, S_max)[:, dead] = 0x7F
        vb[nc:].view(torch.float32).view(KV, S_max)[:, dead] = float("nan")
        assert torch.equal(got, _run(nat, q.cuda(), kb.cuda(), vb.cuda(), n, pos0, H, KV, S_max, W))


def test_model_logits_against_the_oracle(nat):
    """test_gpu_kv_fp8's scenario (40-token prefill, 24 steps, a 300-token prefill at context 64, 8 steps; same seeds, same oracle, same bound) with kv_fp8_chunk:
    the prefills run the fused kernel, the second one against existing cache rows; then forward_logits in this mode."""
    Wl = O.make_lm_weights(TL, 44)
    ids = torch.randint(3, TL.vocab, (sum(n for _, n in PHASES),), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    ref = oracle_logits(Wl, ids, True)
    s = _tiny_model(nat, Wl, kv_fp8=True, kv_fp8_chunk=True).open_stream(max_frames=8, max_seq=1024)
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
    lg = s.forward_logits(ids[:70].cuda())
    assert lg.shape == (70, TL.vocab) and torch.isfinite(lg).all() and s.kv_len == done + 70


def test_refusals(nat):
    lib, z = nat._lib.load(), torch.zeros(64 * 3 * 132, dtype=torch.uint8, device="cuda")
    m = _tiny_model(nat, O.make_lm_weights(TL, 44))
    assert lib.sm_model_set_kv_fp8_chunk(m.h, 1) == -1 and b"kv_fp8" in lib.sm_last_error()
    assert lib.sm_model_set_kv_fp8(m.h, 1) == 0 and lib.sm_model_set_kv_fp8_chunk(m.h, 2) == -1 and lib.sm_model_set_kv_fp8_chunk(m.h, 1) == 0
    assert lib.sm_llm_attention_fp8(z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 0, 3, 1, 128, 64, 0, None, 0, z.data_ptr(), None) == -1 and b"H / KV = 3" in lib.sm_last_error()
