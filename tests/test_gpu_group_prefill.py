"""Batched ragged prefill of a stream group (sm_group_llm_prefill): the ragged attention operator against fp64 softmax attention per stream, the ragged RoPE +
append against sm_rope_kv_append per stream byte for byte, the model call against sm_llm_prefill per stream (logits, then ids on planted margins), the fp8-cache
fallback, and MultiStreamSession(batched_prefill=True) against the per-stream prefills."""
import ctypes as C
import dataclasses

import pytest
import torch

from oracle import streammind_oracle as O
from oracle.make_golden import TINY_V as TV, TINY_C as TC, TINY_G as TG, TINY_L as TL
from tests.test_gpu_kv_fp8 import WIDE, _st, _tiny_model, nat, rnd          # noqa: F401  (nat: the module's fixture)
from tests.test_gpu_kv_fp8_chunk import ref_chunk
from tests.util_models import LOGIT_TOL

pytestmark = pytest.mark.gpu
MANY = [(1 + t % 9, (t * 37) % 501) for t in range(40)]
ATTN_CASES = [([(1, 0)], 32, 8, 0), ([(5, 0), (33, 31), (16, 3000)], 32, 8, 0), ([(130, 62), (40, 1000)], 32, 8, 0), ([(70, 200)], 2, 1, 0), ([(40, 20)], 2, 2, 0),
              ([(20, 100)], 8, 1, 0), ([(40, 100), (16, 300)], 32, 8, 33), (MANY, 32, 8, 0)]


def pack16(k, v, cap, dt):
    """k, v [nk][KV][128] -> the 16-bit cache layout: K [cap][KV*128], V^T [KV*128][cap], the rest of the capacity zero"""
    nk, KV, _ = k.shape
    kb, vb = torch.zeros(cap, KV * 128, dtype=dt), torch.zeros(KV * 128, cap, dtype=dt)
    kb[:nk] = k.reshape(nk, -1).to(dt)
    vb[:, :nk] = v.reshape(nk, -1).t().to(dt)
    return kb, vb


def _tables(segs, bufs):
    """device tables of a launch: seg int32 [S][4] and the two pointer arrays"""
    return (torch.tensor(segs, dtype=torch.int32).cuda(), *(torch.tensor([b[j].data_ptr() for b in bufs], dtype=torch.int64).cuda() for j in (0, 1)))


@pytest.fixture(scope="module")
def kv4k():
    k, v = rnd((3072, 8, 128), 7), rnd((3072, 8, 128), 8)
    k[:, :, :4] *= 6                                            # a few dominant dims, as rotated keys have
    return k, v


@pytest.mark.parametrize("case,f16", [(c, False) for c in range(len(ATTN_CASES))] + [(c, True) for c in range(3)])
def test_ragged_attention(nat, kv4k, case, f16):
    lens, H, KV, W = ATTN_CASES[case]
    lib, dt = nat._lib.load(), torch.float16 if f16 else torch.bfloat16
    gap, segs, row = 3, [], 2                                   # rows of no stream in front of, between and behind the streams'
    for t, (n, pos0) in enumerate(lens):
        segs.append([row, n, pos0, -(-(pos0 + n) // 64) * 64 + 64 * (t % 3)])          # streams have different capacities
        row += n + (gap if t % 2 == 0 else 0)
    rows = row + 1
    q = rnd((rows, H, 128), 60 + case).to(dt)
    host, dev = {}, {}                                          # streams at one (position, capacity) share one cache
    for _, n, pos0, cap in segs:
        if (pos0 + n, cap) not in host:
            host[(pos0 + n, cap)] = pack16(kv4k[0][:pos0 + n, :KV], kv4k[1][:pos0 + n, :KV], cap, dt)
            dev[(pos0 + n, cap)] = tuple(b.cuda() for b in host[(pos0 + n, cap)])
    keys = [(s[2] + s[1], s[3]) for s in segs]
    seg_d, kt, vt = _tables(segs, [dev[k] for k in keys])
    ws = torch.empty(16 * 1024 * 130, device="cuda")
    work = torch.zeros(2 * (rows + len(segs)), dtype=torch.int32)
    n_work, splits = C.c_int(), C.c_int()
    assert lib.sm_llm_attention_ragged_plan(torch.tensor(segs, dtype=torch.int32).data_ptr(), len(segs), rows, H, KV, W, ws.numel(), work.data_ptr(), rows + len(segs),
                                            C.byref(n_work), C.byref(splits)) == 0, lib.sm_last_error()
    if case in (1, 2):
        assert splits.value > 1                                 # a short chunk behind a long context is split over its keys
    work_d, qd = work.cuda(), q.cuda()

    def run():
        ctx = torch.zeros(rows, H, 128, dtype=dt, device="cuda")
        assert lib.sm_llm_attention_ragged(qd.data_ptr(), kt.data_ptr(), vt.data_ptr(), seg_d.data_ptr(), work_d.data_ptr(), n_work.value, rows, H, KV, 128, W, int(f16),
                                           ws.data_ptr(), ws.numel(), splits.value, ctx.data_ptr(), _st()) == 0, lib.sm_last_error()
        torch.cuda.synchronize()
        return [ctx[r0:r0 + n].cpu() for r0, n, _, _ in segs]
    got = run()
    for (r0, n, pos0, cap), key, o in zip(segs, keys, got):
        kb, vb = host[key]
        kd, vd = kb[:pos0 + n].view(-1, KV, 128).double(), vb[:, :pos0 + n].t().reshape(-1, KV, 128).double()
        ref = ref_chunk(q[r0:r0 + n], kd, vd, pos0, W)
        assert ((o.double() - ref).abs().max() / ref.abs().max()).item() < 8e-3, (r0, n, pos0)
    # NaN patterns in every dead cache position (behind a stream's newest row; in front of the window of its first row) and in the q rows of no stream
    live = torch.zeros(rows, dtype=torch.bool)
    for (r0, n, pos0, cap), key in zip(segs, keys):
        live[r0:r0 + n] = True
        kb, vb = dev[key]
        kb[pos0 + n:] = float("nan"); vb[:, pos0 + n:] = float("nan")
    if W:
        for (r0, n, pos0, cap), key in zip(segs, keys):
            dead = max(0, pos0 - W + 1)
            dev[key][0][:dead] = float("nan"); dev[key][1][:, :dead] = float("nan")
    qd[~live.cuda()] = float("nan")
    assert all(torch.equal(a, b) for a, b in zip(got, run()))


def test_ragged_append_equals_per_stream_append(nat):
    lib, H, KV = nat._lib.load(), 4, 2
    lens = [(5, 0), (33, 31), (130, 62)]
    cfg = dataclasses.replace(TL, hidden=H * 128, heads=H, kv_heads=KV)
    cos, sin = (t[:, :64].contiguous().cuda() for t in O.rope_cos_sin(torch.arange(320), cfg))
    segs, row = [], 0
    for t, (n, pos0) in enumerate(lens):
        segs.append([row, n, pos0, 192 + 64 * t])
        row += n
    qkv = rnd((row, (H + 2 * KV) * 128), 17).cuda()
    new = lambda: [tuple(torch.full((cap * KV * 256,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)) for *_, cap in segs]
    q1, q2 = (torch.full((row, H * 128), 7.0, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    b1, b2 = new(), new()
    seg_d, kt, vt = _tables(segs, b1)
    tiles = torch.tensor([[s, r] for s, (n, _) in enumerate(lens) for r in range(0, n, 64)], dtype=torch.int32).cuda()
    assert lib.sm_rope_kv_append_ragged(qkv.data_ptr(), seg_d.data_ptr(), tiles.data_ptr(), tiles.shape[0], H, KV, cos.data_ptr(), sin.data_ptr(), q1.data_ptr(),
                                        kt.data_ptr(), vt.data_ptr(), 0, _st()) == 0, lib.sm_last_error()
    for (r0, n, pos0, cap), (kb, vb) in zip(segs, b2):
        assert lib.sm_rope_kv_append(qkv[r0:r0 + n].data_ptr(), n, pos0, H, KV, 128, cos.data_ptr(), sin.data_ptr(), q2[r0:r0 + n].data_ptr(), kb.data_ptr(), vb.data_ptr(),
                                     cap, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(q1, q2)
    for (r0, n, pos0, cap), a, b in zip(segs, b1, b2):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        k2, v2 = a[0].view(cap, -1), a[1].view(KV * 128, cap * 2)
        assert (k2[:pos0] == 0x5A).all() and (k2[pos0 + n:] == 0x5A).all() and (v2[:, :2 * pos0] == 0x5A).all() and (v2[:, 2 * (pos0 + n):] == 0x5A).all()
        assert not (k2[pos0:pos0 + n] == 0x5A).all()


@pytest.mark.parametrize("ctx,new", [((0, 40, 300), (7, 0, 70)), ((10, 0), (1500, 700))])
def test_model_logits_equal_solo_prefill(nat, ctx, new):
    """group prefill against a twin stream driven by prefill alone; second case: 2200 rows, the pass boundary (2048) falls inside the second stream"""
    m = _tiny_model(nat, O.make_lm_weights(TL, 44))
    g = torch.Generator().manual_seed(9)
    ids = lambda n: torch.randint(3, TL.vocab, (n,), generator=g, dtype=torch.int32).cuda()
    grp, solo = ([m.open_stream(max_frames=8, max_seq=2304) for _ in ctx] for _ in range(2))
    for c, a, b in zip(ctx, grp, solo):
        if c:
            x = ids(c)
            a.prefill(x); b.prefill(x)
    before = [(s.kv_len, s.logits()[0].clone(), s.state()) for s in grp]
    xs = [ids(n) if n else None for n in new]
    m.open_group(grp).prefill(xs)
    for t, (n, a, b) in enumerate(zip(new, grp, solo)):
        if n:
            b.prefill(xs[t])
            assert a.kv_len == b.kv_len == ctx[t] + n
            assert (a.logits()[0] - b.logits()[0]).abs().max().item() < LOGIT_TOL, t
        else:
            assert a.kv_len == before[t][0] and torch.equal(a.logits()[0], before[t][1]) and all(torch.equal(u, v) for u, v in zip(a.state(), before[t][2]))


@pytest.mark.parametrize("S,cfgs", [(3, (TC, TG, TL)), (70, WIDE)])
def test_model_group_prefill_then_decode_equals_solo(nat, S, cfgs):
    """planted-margin weights: group prefill + group decode emit exactly the ids of solo prefill + solo decode (every solo step's margin above 4 x the tolerance)"""
    from tests.test_gpu_parity_full import _planted_llm
    m = _tiny_model(nat, _planted_llm(cfgs[2], 808, peak=16.0)[0], cfgs)
    g = torch.Generator().manual_seed(12)
    ctxs = [torch.randint(3, cfgs[2].vocab, (int(torch.randint(5, 60, (1,), generator=g)),), generator=g, dtype=torch.int32).cuda() for _ in range(S)]
    want = []
    for c in ctxs:
        s = m.open_stream(max_frames=8, max_seq=128)
        s.prefill(c)
        want.append([])
        for _ in range(8):
            assert float(torch.topk(s.logits()[0], 2).values.diff().abs()) > 4 * LOGIT_TOL
            want[-1].append(int(s.decode(1)[0]))
    grp = m.open_group([m.open_stream(max_frames=8, max_seq=128) for _ in ctxs])
    grp.prefill(ctxs)
    assert grp.decode(8).cpu().tolist() == want


def test_fp8_cache_falls_back_to_solo_prefill(nat):
    m = _tiny_model(nat, O.make_lm_weights(TL, 44), kv_fp8=True)
    xs = [torch.randint(3, TL.vocab, (n,), generator=torch.Generator().manual_seed(n), dtype=torch.int32).cuda() for n in (40, 9)]
    grp, solo = ([m.open_stream(max_frames=8, max_seq=128) for _ in xs] for _ in range(2))
    m.open_group(grp).prefill(xs)
    for a, b, x in zip(grp, solo, xs):
        b.prefill(x)
        assert a.kv_len == b.kv_len and torch.equal(a.logits()[0], b.logits()[0])


def test_session_batched_prefill_equals_per_stream_prefill(nat, tiny_tokenizer):
    from streammind_amd.model import Videollama2MistralForCausalLM
    from streammind_amd.stream import MultiStreamSession
    from tests.test_gpu_parity_full import _planted_llm
    m = _tiny_model(nat, _planted_llm(TL, 808, peak=16.0)[0])
    S, T = 6, 8
    frames = torch.stack([O.synthetic_frames(T, TV.image_size, seed=500 + s, scene_len=3) for s in range(S)])
    runs = []
    for batched in (False, True):
        models = [Videollama2MistralForCausalLM(m, max_frames=32, max_seq=512, eos_token_id=tiny_tokenizer.eos_token_id) for _ in range(S)]
        sess = MultiStreamSession(models, tiny_tokenizer, max_new_tokens=6, decode_chunk=4, batched_prefill=batched)
        ticks = [[(i, e.frame_index, e.text, e.new_ids) for i, e in sess.tick(frames[:, t])] for t in range(T)]
        runs.append((ticks, sess.prompts))
    assert max(len(t) for t in runs[0][0]) >= 2                # several streams fire in one tick
    assert runs[0] == runs[1]
