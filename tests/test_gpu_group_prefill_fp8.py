"""Batched ragged prefill over the FP8 K / V cache (kv_fp8 + kv_fp8_chunk): sm_llm_attention_ragged_fp8 against fp64 softmax attention over the SAME dequantised
caches (NaN codes and NaN scales wherever it may not look) and bit for bit against sm_llm_attention_fp8, sm_rope_kv_append_fp8_ragged byte for byte against
sm_rope_kv_append_fp8 per stream, and the model call against solo prefill (logits, then ids on planted margins)."""
import ctypes as C
import dataclasses

import pytest
import torch

from oracle import streammind_oracle as O
from oracle.make_golden import TINY_C as TC, TINY_G as TG, TINY_L as TL
from tests.test_gpu_kv_fp8 import WIDE, _st, _tiny_model, nat, pack_cache, rnd  # noqa: F401  (nat: the module's fixture)
from tests.test_gpu_kv_fp8_chunk import ref_chunk
import tests.test_gpu_group_prefill as G
from tests.test_gpu_group_prefill import ATTN_CASES, _tables, kv4k     # noqa: F401  (kv4k: that module's fixture, k / v fp32 [3072][8][128]; the last case: its MANY)

pytestmark = pytest.mark.gpu


def _plan(lib, segs, rows, H, KV, W, ws_floats):
    work, n_work, splits = torch.zeros(2 * (rows + len(segs)), dtype=torch.int32), C.c_int(), C.c_int()
    assert lib.sm_llm_attention_ragged_plan(torch.tensor(segs, dtype=torch.int32).data_ptr(), len(segs), rows, H, KV, W, ws_floats, work.data_ptr(), rows + len(segs),
                                            C.byref(n_work), C.byref(splits)) == 0, lib.sm_last_error()
    return work.cuda(), n_work.value, splits.value


@pytest.mark.parametrize("case", range(len(ATTN_CASES)))
def test_ragged_attention_fp8(nat, kv4k, case):
    lens, H, KV, W = ATTN_CASES[case]
    lib, gap, segs, row = nat._lib.load(), 3, [], 2             # rows of no stream in front of, between and behind the streams'
    for t, (n, pos0) in enumerate(lens):
        segs.append([row, n, pos0, -(-(pos0 + n) // 64) * 64 + 64 * (t % 3)])          # streams have different capacities
        row += n + (gap if t % 2 == 0 else 0)
    rows = row + 1
    q = rnd((rows, H, 128), 60 + case).bfloat16()
    host, dev = {}, {}                                          # streams at one (position, capacity) share one cache
    for _, n, pos0, cap in segs:
        if (pos0 + n, cap) not in host:
            host[(pos0 + n, cap)] = pack_cache(kv4k[0][:pos0 + n, :KV], kv4k[1][:pos0 + n, :KV], cap)
            dev[(pos0 + n, cap)] = tuple(b.cuda() for b in host[(pos0 + n, cap)][:2])
    keys = [(s[2] + s[1], s[3]) for s in segs]
    seg_d, kt, vt = _tables(segs, [dev[k] for k in keys])
    ws = torch.empty(16 * 1024 * 130, device="cuda")
    work_d, n_work, splits = _plan(lib, segs, rows, H, KV, W, ws.numel())
    if case in (1, 2):
        assert splits > 1                                       # a short chunk behind a long context is split over its keys
    qd = q.cuda()

    def run():
        ctx = torch.zeros(rows, H, 128, dtype=torch.bfloat16, device="cuda")
        assert lib.sm_llm_attention_ragged_fp8(qd.data_ptr(), kt.data_ptr(), vt.data_ptr(), seg_d.data_ptr(), work_d.data_ptr(), n_work, rows, H, KV, 128, W,
                                               ws.data_ptr(), ws.numel(), splits, ctx.data_ptr(), _st()) == 0, lib.sm_last_error()
        torch.cuda.synchronize()
        return [ctx[r0:r0 + n].cpu() for r0, n, _, _ in segs]
    got = run()
    for (r0, n, pos0, cap), key, o in zip(segs, keys, got):
        ref = ref_chunk(q[r0:r0 + n], host[key][2], host[key][3], pos0, W)
        err = ((o.double() - ref).abs().max() / ref.abs().max()).item()
        print(f"ragged_attn_fp8 case {case} stream {(n, pos0, cap)}: rel err {err:.2e}")
        assert err < 8e-3, (r0, n, pos0)
    # code 0x7F and NaN scales in every dead cache position (behind a stream's newest row; in front of the window of its first row), NaN in the q rows of no stream
    live = torch.zeros(rows, dtype=torch.bool)
    for (r0, n, pos0, cap), key in zip(segs, keys):
        live[r0:r0 + n] = True
        kb, vb = dev[key]
        nc, dead = cap * KV * 128, (torch.arange(cap) >= pos0 + n) | ((torch.arange(cap) < pos0 - W + 1) & (W > 0))
        kb[:nc].view(cap, KV * 128)[dead.cuda()] = 0x7F
        kb[nc:].view(torch.float32).view(cap, KV)[dead.cuda()] = float("nan")
        vb[:nc].view(KV * 128, cap)[:, dead.cuda()] = 0x7F
        vb[nc:].view(torch.float32).view(KV, cap)[:, dead.cuda()] = float("nan")
    qd[~live.cuda()] = float("nan")
    assert all(torch.equal(a, b) for a, b in zip(got, run()))


@pytest.mark.parametrize("n,pos0,W", [(33, 31, 0), (130, 62, 0), (40, 100, 33)])
def test_one_stream_one_split_equals_the_chunk_kernel(nat, kv4k, n, pos0, W):
    lib, H, KV, cap = nat._lib.load(), 32, 8, 256
    kb, vb = (b.cuda() for b in pack_cache(kv4k[0][:pos0 + n], kv4k[1][:pos0 + n], cap)[:2])
    q = rnd((n, H, 128), 77).bfloat16().cuda()
    segs = [[0, n, pos0, cap]]
    seg_d, kt, vt = _tables(segs, [(kb, vb)])
    work_d, n_work, splits = _plan(lib, segs, n, H, KV, W, 0)
    assert splits == 1
    a, b = (torch.zeros(n, H, 128, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    assert lib.sm_llm_attention_ragged_fp8(q.data_ptr(), kt.data_ptr(), vt.data_ptr(), seg_d.data_ptr(), work_d.data_ptr(), n_work, n, H, KV, 128, W, None, 0, 1,
                                           a.data_ptr(), _st()) == 0, lib.sm_last_error()
    assert lib.sm_llm_attention_fp8(q.data_ptr(), kb.data_ptr(), vb.data_ptr(), n, pos0, H, KV, 128, cap, W, None, 0, b.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_ragged_append_fp8_equals_per_stream_append(nat):
    lib, H, KV = nat._lib.load(), 4, 2
    lens = [(5, 0), (33, 31), (130, 62)]
    cfg = dataclasses.replace(TL, hidden=H * 128, heads=H, kv_heads=KV)
    cos, sin = (t[:, :64].contiguous().cuda() for t in O.rope_cos_sin(torch.arange(320), cfg))
    segs, row = [], 0
    for t, (n, pos0) in enumerate(lens):
        segs.append([row, n, pos0, 192 + 64 * t])
        row += n
    qkv = rnd((row, (H + 2 * KV) * 128), 17).cuda()
    new = lambda: [tuple(torch.full((cap * KV * 132,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)) for *_, cap in segs]
    q1, q2 = (torch.full((row, H * 128), 7.0, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    b1, b2 = new(), new()
    seg_d, kt, vt = _tables(segs, b1)
    tiles = torch.tensor([[s, r] for s, (n, _) in enumerate(lens) for r in range(0, n, 64)], dtype=torch.int32).cuda()
    assert lib.sm_rope_kv_append_fp8_ragged(qkv.data_ptr(), seg_d.data_ptr(), tiles.data_ptr(), tiles.shape[0], H, KV, cos.data_ptr(), sin.data_ptr(), q1.data_ptr(),
                                            kt.data_ptr(), vt.data_ptr(), _st()) == 0, lib.sm_last_error()
    for (r0, n, pos0, cap), (kb, vb) in zip(segs, b2):
        assert lib.sm_rope_kv_append_fp8(qkv[r0:r0 + n].data_ptr(), n, pos0, H, KV, 128, cos.data_ptr(), sin.data_ptr(), q2[r0:r0 + n].data_ptr(), kb.data_ptr(), vb.data_ptr(),
                                         cap, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(q1, q2)
    for (r0, n, pos0, cap), a, b in zip(segs, b1, b2):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        nc, out = cap * KV * 128, torch.ones(cap, dtype=torch.bool, device="cuda")
        out[pos0:pos0 + n] = False                              # every byte outside the appended positions, codes and scales, is untouched
        assert (a[0][:nc].view(cap, -1)[out] == 0x5A).all() and (a[0][nc:].view(cap, -1)[out] == 0x5A).all()
        assert (a[1][:nc].view(KV * 128, cap)[:, out] == 0x5A).all() and (a[1][nc:].view(KV, cap, 4)[:, out] == 0x5A).all()
        assert not (a[0][:nc].view(cap, -1)[~out] == 0x5A).all()


@pytest.fixture
def fp8_models(monkeypatch):
    """the model scenarios of test_gpu_group_prefill, their models built with the FP8 cache read directly by multi-row calls"""
    monkeypatch.setattr(G, "_tiny_model", lambda *a, **kw: _tiny_model(*a, kv_fp8=True, kv_fp8_chunk=True, **kw))


@pytest.mark.parametrize("ctx,new", [((0, 40, 300), (7, 0, 70)), ((10, 0), (1500, 700))])
def test_model_logits_equal_solo_prefill(nat, fp8_models, ctx, new):
    """kv_len equal, logits within LOGIT_TOL of twin streams driven by solo prefill (measured: 0 and, where the 2048-row pass boundary cuts the second stream,
    8.3e-3), the non-participating stream untouched"""
    G.test_model_logits_equal_solo_prefill(nat, ctx, new)


@pytest.mark.parametrize("S,cfgs", [(3, (TC, TG, TL)), (70, WIDE)])
def test_model_group_prefill_then_decode_equals_solo(nat, fp8_models, S, cfgs):
    """planted-margin weights: group prefill + group decode emit exactly the ids of solo prefill + solo decode"""
    G.test_model_group_prefill_then_decode_equals_solo(nat, S, cfgs)


def test_refusal(nat):
    lib, z = nat._lib.load(), torch.zeros(64 * 3 * 132, dtype=torch.uint8, device="cuda")
    assert lib.sm_llm_attention_ragged_fp8(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 1, 3, 1, 128, 0, None, 0, 1, z.data_ptr(), None) == -1
    assert b"H / KV = 3" in lib.sm_last_error()
