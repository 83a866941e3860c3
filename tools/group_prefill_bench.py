"""Batched ragged prefill (sm_group_llm_prefill) against one sm_llm_prefill per stream, and the ragged attention kernel with one stream against the chunk
attention of the 16-bit cache -- Mistral-7B widths, bf16, ONE process, the legs alternating over the rounds; prints one JSON line:
  group_prefill_ms   ms per call (host clock around `reps` calls ending in a synchronise) for S = 8 and 32 streams x 32 new ids behind a context of 2048 tokens:
                     `serial` = the S streams prefilled one by one, `group` = one group prefill; every call starts from kv_len 2048 again
  chunk_attn_us      HIP-event time of one layer's attention for (n, pos0) = (16, 4080) and (64, 4032), H = 32, KV = 8, capacity 4096: `prefill` = sm_llm_attention,
                     `ragged` = sm_llm_attention_ragged with S = 1 incl. its split merge (the plan is made once, outside the bracket); 200 calls per bracket
With `fp8` the model holds the FP8 K / V cache with kv_fp8_chunk (the batched pass runs sm_rope_kv_append_fp8_ragged + sm_llm_attention_ragged_fp8; `serial` is
what the group call did for this model before that pass existed) and chunk_attn_us times `fused` = sm_llm_attention_fp8 against `ragged` =
sm_llm_attention_ragged_fp8.

    python tools/group_prefill_bench.py [rounds] [fp8]"""
import ctypes as C
import json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.kv_fp8_bench import make_model


def chunk_attn_us(lib, rounds, fp8=False):
    H, KV, cap = 32, 8, 4096
    g = torch.Generator(device="cuda").manual_seed(3)
    if fp8:                                                   # finite codes, scales 2^-6 (tools/kv_fp8_bench.py's cache)
        kb, vb = (torch.randint(0, 0x78, (cap * KV * 132,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2))
        for b in (kb, vb):
            b[cap * KV * 128:].view(torch.float32).fill_(2.0 ** -6)
    else:
        kb, vb = (torch.randn(cap * KV * 128, device="cuda", generator=g).bfloat16() for _ in range(2))
    q = torch.randn(64, H * 128, device="cuda", generator=g).bfloat16()
    ctx, ws = torch.empty_like(q), torch.empty(2048 * H * 130, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    kt, vt = (torch.tensor([b.data_ptr()], dtype=torch.int64).cuda() for b in (kb, vb))
    out = {}
    for n, pos0 in ((16, 4080), (64, 4032)):
        seg = torch.tensor([0, n, pos0, cap], dtype=torch.int32)
        work, nw, sp = torch.zeros(2 * (n + 1), dtype=torch.int32), C.c_int(), C.c_int()
        assert lib.sm_llm_attention_ragged_plan(P(seg), 1, n, H, KV, 0, ws.numel(), P(work), n + 1, C.byref(nw), C.byref(sp)) == 0
        seg_d, work_d = seg.cuda(), work.cuda()
        legs = {"prefill": lambda: lib.sm_llm_attention(P(q), P(kb), P(vb), n, pos0, H, KV, 128, cap, P(ctx), st),
                "ragged": lambda: lib.sm_llm_attention_ragged(P(q), P(kt), P(vt), P(seg_d), P(work_d), nw.value, n, H, KV, 128, 0, 0, P(ws), ws.numel(), sp.value, P(ctx), st)}
        if fp8:
            legs = {"fused": lambda: lib.sm_llm_attention_fp8(P(q), P(kb), P(vb), n, pos0, H, KV, 128, cap, 0, P(ws), ws.numel(), P(ctx), st),
                    "ragged": lambda: lib.sm_llm_attention_ragged_fp8(P(q), P(kt), P(vt), P(seg_d), P(work_d), nw.value, n, H, KV, 128, 0, P(ws), ws.numel(), sp.value, P(ctx), st)}
        per = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                assert fn() == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    fn()
                e1.record(); torch.cuda.synchronize()
                per[name].append(round(e0.elapsed_time(e1) * 1e3 / 200, 2))
        out[f"{n}@{pos0}"] = {"splits": sp.value, **{name: {"median": statistics.median(v), "runs": v} for name, v in per.items()}}
    return out


def main(rounds=3, fp8=False):
    cfg, m = make_model(kv_fp8=True, kv_fp8_chunk=True) if fp8 else make_model()
    g = torch.Generator(device="cuda").manual_seed(17)
    ids = lambda n: torch.randint(3, 32000, (n,), generator=g, device="cuda", dtype=torch.int32)
    res = {"group_prefill_ms": {}, "chunk_attn_us": chunk_attn_us(m.lib, rounds, fp8)}
    streams = [m.open_stream(max_frames=8, max_seq=2304) for _ in range(32)]
    ctx = ids(2048)
    for s in streams:
        s.prefill(ctx)
    new = [ids(32) for _ in streams]
    for S in (8, 32):
        grp, reps = m.open_group(streams[:S]), {"serial": 64 // S, "group": 48}          # windows of 0.25 s and more

        def serial():
            for s, x in zip(streams[:S], new):
                s.set_kv_len(2048); s.prefill(x)

        def group():
            for s in streams[:S]:
                s.set_kv_len(2048)
            grp.prefill(new[:S])
        per = {"serial": [], "group": []}
        for _ in range(rounds):
            for name, fn in (("serial", serial), ("group", group)):
                fn(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps[name]):
                    fn()
                torch.cuda.synchronize()
                per[name].append(round((time.perf_counter() - t0) / reps[name] * 1e3, 3))
        res["group_prefill_ms"][f"{S}x32@2048"] = {name: {"median": statistics.median(v), "runs": v} for name, v in per.items()}
        grp.close()
    print(json.dumps(res))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "fp8"]
    main(int(args[0]) if args else 3, "fp8" in sys.argv[1:])
